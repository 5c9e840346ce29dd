/*
 * pyg_hip.h -- C-ABI of the MI355X-native (gfx950) pyg-lib hot path.
 *
 * This is the drop-in boundary: a torch-free shared library (libpyg_hip.so) with plain
 * pointers, sizes and a hipStream_t.  The thin torch binding (libpyg.so, sources in
 * pyg_lib_amd/csrc/binding/) registers the reference's `pyg::*` operator schemas and calls
 * nothing but these entry points; INTEGRATION.md shows the binding a pyg-lib maintainer
 * would add.  Every entry point cites the reference interface it replaces
 * (paths relative to the pyg-lib source tree, v0.9.0).
 *
 * Conventions
 *  - every function returns PYG_HIP_OK (0) or a negative pyg_hip_status; no exception crosses
 *    this boundary.  pyg_hip_last_error() returns a thread-local message for the last failure
 *    (the binding turns it into TORCH_CHECK -> RuntimeError, the reference's error convention:
 *    pyg_lib/csrc/ops/matmul.cpp:14-32,49-55).
 *  - all data pointers are DEVICE pointers unless the name ends in `_host`.
 *  - inputs are borrowed and never written; outputs are caller-allocated, or allocated through
 *    the caller's allocator callback when their size is data dependent (sampler).
 *  - `stream` is a hipStream_t passed as void* so that C callers need no HIP headers.  All work
 *    is enqueued on it; only the sampler synchronises it (data-dependent output sizes).
 */
#ifndef PYG_HIP_H_
#define PYG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYG_HIP_API __attribute__((visibility("default")))

typedef enum {
  PYG_HIP_OK = 0,
  PYG_HIP_ERR_INVALID = -1,     /* argument check failed (reference: TORCH_CHECK)          */
  PYG_HIP_ERR_UNSUPPORTED = -2, /* valid in the reference, not implemented on device yet     */
  PYG_HIP_ERR_RUNTIME = -3,     /* HIP runtime / launch failure                              */
  PYG_HIP_ERR_WORKSPACE = -4    /* workspace too small                                       */
} pyg_hip_status;

/* Arithmetic type of a buffer (AT_DISPATCH_ALL_TYPES_AND2(Half, BFloat16),
 * pyg_lib/csrc/ops/cpu/matmul_kernel.cpp:419-421). */
typedef enum {
  PYG_F32 = 0,
  PYG_F64 = 1,
  PYG_F16 = 2,
  PYG_BF16 = 3,
  PYG_I8 = 4,
  PYG_U8 = 5,
  PYG_I16 = 6,
  PYG_I32 = 7,
  PYG_I64 = 8
} pyg_dtype;

/* ---- library ----------------------------------------------------------------------------- */

/* Version of THIS interface: bumped whenever a signature or the meaning of an argument changes, so that a caller built
 * against an older header can tell (pyg_hip_abi_version() != the PYG_HIP_ABI_VERSION it was compiled with).
 *  21: pyg_hip_edge_lookup, pyg_hip_negative_sample (edge membership on a CSR graph and exact uniform draws over its
 *      non-edges, keyed and deterministic).
 *  20: pyg_hip_rgcn_route, pyg_hip_rgcn_last_route (which kernel family serves a fused R-GCN call: asked without running,
 *      told after).
 *  19: pyg_hip_node2vec_walk (second-order (p, q) random walks, keyed and deterministic).
 *  18: pyg_hip_csr_route, pyg_hip_csr_last_route (which kernels serve a CSR reduction, gather or softmax: asked without
 *      running, told after).
 *  17: pyg_hip_graclus / _graclus_route / _graclus_last_route / _graclus_tile / _graclus_workspace_size / _graclus_pending_error
 *      (greedy graph matching in parallel rounds).
 *  16: pyg_hip_spline_basis / _basis_backward / _weighting / _weighting_backward_x / _weighting_backward_weight /
 *      _weighting_backward_basis, pyg_hip_spline_backward_x_workspace_size / _backward_weight_workspace_size,
 *      pyg_hip_spline_route / _last_route / _tile / _pending_error (the operators behind SplineConv).
 *  15: pyg_hip_fps / _fps_route / _fps_last_route / _fps_tile / _fps_workspace_size / _fps_pending_error, pyg_hip_grid_cluster /
 *      _grid_cluster_workspace_size (point-cloud downsampling).
 *  14: pyg_hip_matmul_dw_route (which weight-gradient kernel serves a call, asked without running); a host `ptr` of
 *      pyg_hip_segment_matmul_dw is validated, pyg_hip_matmul_dw_counters count calls that returned PYG_HIP_OK.
 *  13: pyg_hip_knn / _knn_emit, pyg_hip_radius / _radius_emit, pyg_hip_nearest, pyg_hip_spatial_route / _last_route / _tile /
 *      _workspace_size, pyg_hip_nearest_pending_error (batched point-cloud neighbour search).
 *  12: pyg_hip_scatter_route, pyg_hip_scatter_last_route (which kernel serves a scatter call: asked without running, told after).
 *  11: pyg_hip_fused_scatter_reduce, its _workspace_size and _backward (sum / mean / min / max in one sort and one pass).
 *  10: pyg_hip_sampled_op, pyg_hip_sampled_op_backward (fused gather + binary operator and its per-edge gradients).
 *   9: pyg_hip_random_walk, pyg_hip_subgraph (added after the original hot-path contract).
 *   8: round 6 -- pyg_hip_segment_csr_ws / pyg_hip_gather_csr_ws / pyg_hip_csr_hub_workspace_size (scratch for hub rows);
 *      pyg_hip_scatter uses the dead parts of its workspace for the same purpose (no change for its callers).
 *   7: round 6 -- pyg_hip_rgcn_relation::scatter_rows (rows of the relation's destination segment).
 *   6: round 5 -- PYG_HIP_RGCN_GROUPED + pyg_hip_rgcn_grouped_workspace_size (atomic-free fused layer), PYG_HIP_SCATTER_DETERMINISTIC.
 *   5: round 5 -- pyg_hip_hetero_neighbor_sample_batched, PYG_HIP_SCATTER_CAS / PYG_HIP_RGCN_* flag bits (`checked` of
 *      pyg_hip_rgcn_fused became a bit field), pyg_hip_set_float_atomic_mode, pyg_hip_atomic_selftest,
 *      pyg_hip_sampler_table_cache_release; the weight-gradient workspace holds partial slabs instead of an fp32 image.
 *   4: round 4 -- `flags` in front of `stream` in pyg_hip_segment_matmul / pyg_hip_grouped_matmul, `index_sorted` of
 *      pyg_hip_scatter became a bit field, pyg_hip_matmul_set_schedule / _set_f32_split removed, fp32 default = IEEE MFMAs. */
#define PYG_HIP_ABI_VERSION 21
PYG_HIP_API int pyg_hip_abi_version(void);
/* Replaces pyg::cuda_version (pyg_lib/csrc/library.cpp:19-29): returns the HIP runtime version
 * the library was built against (HIP_VERSION), never -1. */
PYG_HIP_API int64_t pyg_hip_version(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
PYG_HIP_API const char* pyg_hip_last_error(void);
/* Name of the offload architecture the kernels were compiled for ("gfx950"). */
PYG_HIP_API const char* pyg_hip_arch(void);

/*
 * Floating-point accumulation through atomics.  The weight gradients, the large scatter / COO sums and the CSR family are
 * atomic-free and bit-reproducible (as the reference's sequential CPU loops, ops/cpu/scatter_kernel.cpp:29-127,
 * ops/autograd/matmul_kernel.cpp:92-107).  What still adds through atomics -- small or element-wise indexed
 * scatter sums, float64 sums, pyg_hip_rgcn_fused -- uses the hardware's floating-point atomic adds by default
 * (global_atomic_add_f32 / _f64 / _pk_add_bf16 / _pk_add_f16) and can be switched to compare-and-swap loops on the containing
 * word: per call (PYG_HIP_SCATTER_CAS, PYG_HIP_RGCN_CAS) or as the process-wide default below (0 = hardware adds,
 * 1 = CAS loops; initial value from the environment, PYG_HIP_FLOAT_ATOMICS=hw|cas).  Same sums up to the order the adds
 * land in; the CAS form is 1.5 - 3x slower on contended rows.  Returns the previous default.
 * Denormals: both flavours keep them -- measured on gfx950, the hardware adds (f32, f64 and the packed 16-bit pairs) return
 * exact denormal sums bit for bit like the CAS loops, the atomic-free paths and the CPU (tests/test_special_values_gpu.py).
 */
PYG_HIP_API int pyg_hip_set_float_atomic_mode(int mode);
/* What the calling process's LAST launch of an atomically accumulating kernel was (thread-local text buffer): operator,
 * accumulator address / bytes / hipPointerGetAttributes, who cleared it and how, stream, flavour.  For failure reports. */
PYG_HIP_API const char* pyg_hip_last_accumulate_info(void);
/*
 * In-process health check of "clear an accumulator, add to it from all over the chip, read it back" on the CALLER'S memory
 * and stream: 5 add flavours (hw f32 / packed bf16 / f64, CAS f32, int32) x 3 ways of clearing (hipMemsetAsync, fill kernel
 * with plain stores, fill kernel with write-through stores) x 2 readbacks (copy kernel + D2H, D2H), `rounds` times each,
 * the accumulator scribbled with NaN patterns before every round.  `scratch`: >= 64 KiB of 16-byte aligned device memory
 * (up to 16 MiB are used).  Writes a text report (one line per failing variant, classified: NaN = the clear never
 * arrived, low = updates lost / clear late / stale read, high = doubled) and returns the number of failing variants
 * (0 = healthy) or a negative pyg_hip_status.  Synchronises `stream`.
 */
PYG_HIP_API int pyg_hip_atomic_selftest(void* scratch, size_t scratch_bytes, int rounds, char* report, size_t report_cap,
                                        void* stream);

/* ---- segment_matmul / grouped_matmul ------------------------------------------------------ */

/*
 * Per-call mode of pyg_hip_segment_matmul / pyg_hip_grouped_matmul (`flags` argument; 0 = defaults).  The mode is an
 * argument, not process state: calls in flight on different threads (autograd workers next to the main thread) never
 * see each other's choice -- the reference keeps its launch state in unlocked process globals
 * (ops/cuda/matmul_kernel.cu:19,118-119); this build does not.
 *
 * Bits 0-3: tile schedule / kernel family (PYG_HIP_MM_SCHED_*); every choice gives the same bits per output element
 * for the 16-bit types (same k order), they differ in speed only.
 *   AUTO        (default) the ticket schedule once every CU has several tiles to sweep, the item ring for many short
 *               relations (16-bit: fewer than 4096 rows per relation on average; fp32 split-bf16: fewer than 512),
 *               contiguous ranges below that;
 *   CONTIGUOUS  one contiguous tile range per workgroup (mfma_rows_lds_kernel): up to 6.1 TB/s on C2 when the
 *               allocator happened to place input and output favourably, 5.0 TB/s otherwise;
 *   CYCLIC      banded cyclic (mfma_rows_cyc_kernel): 6.2 - 6.3 TB/s on favourably placed buffers, 5.4 - 5.6 otherwise;
 *   TICKET      tiles drawn in address order from per-XCD counters, W in registers (mfma_rows_ticket_kernel):
 *               6.1 - 6.2 TB/s on either placement;
 *   GENERAL     (measurement only) every bf16 / f16 / f32 call through the general-shape MFMA kernel (matmul_gen.hip),
 *               also the shapes that have a specialised kernel;
 *   NAIVE       (measurement only) every call through the one-thread-per-output kernel;
 *   RING        the item-ring kernels (matmul_ring.hip): W slices in registers, X tiles and W chunks through one
 *               LDS-DMA ring: 5.0 - 5.4 TB/s at any segment length, where the ticket kernel falls to 3.0 at 256 rows.
 * 16-bit K = M = 256 has three kernels: AUTO / RING = W in registers + LDS-DMA item ring (mfma_rows_k256_regw_kernel),
 * CONTIGUOUS = W in LDS, 32 rows per wave (mfma_rows_wide256_kernel), CYCLIC / TICKET = W in LDS, 64 rows per wave
 * (mfma_rows_wide256r2_kernel).  The reference has no counterpart (its CUTLASS problem visitor is fixed,
 * ops/cuda/matmul_kernel.cu:121-287).
 *
 * Bit 8, PYG_HIP_MM_F32_SPLIT: arithmetic of the fp32 K = 128, M % 128 == 0 kernels.
 *   clear (default)  v_mfma_f32_32x32x2_f32 (mfma_rows_f32_pipe_kernel): IEEE fp32 products and sums, Inf / NaN / the
 *      whole fp32 range behave as in the reference's CPU kernel; bound by the fp32 matrix rate (157 TFLOP/s).
 *   set   split-bf16: every fp32 operand is split, round-to-nearest, into three bf16 terms (8 + 8 + 8 significant
 *      bits; the split is exact to 2^-27 relative) and the six leading cross products run on v_mfma_f32_32x32x16_bf16
 *      with fp32 accumulation.  Dropped terms: 2^-26 |x||w| per product at most, unbiased -- below the rounding unit
 *      of an fp32 multiply-add; 2.7x less matrix time: the kernel is HBM-bound.  Special values: a NaN operand gives
 *      NaN as it must; a +-Inf operand, or a finite one beyond the largest bf16 (|v| > 3.3895e38), gives NaN in every
 *      output it feeds (first term Inf, residual Inf - Inf) where the exact kernel gives +-Inf / a finite product;
 *      third terms of operands below ~2^-100 fall into the bf16 denormals the matrix unit flushes (those products keep
 *      16 instead of 24 bits).  This is the reduced-guarantee mode in the sense of the reference's TF32 switch: the
 *      torch binding sets the bit only when at::globalContext().float32MatmulPrecision() != HIGHEST, the rule of
 *      ops/cuda/matmul_kernel.cu:158-165 (torch's default is HIGHEST, i.e. the bit is clear unless the user called
 *      torch.set_float32_matmul_precision('high' | 'medium')).  Unlike TF32 the mode keeps full fp32 accuracy on
 *      finite data inside 2^-100 ... 2^127 (relative Frobenius error ~1e-7 against float64, as the exact kernel).
 * Any other bit set: PYG_HIP_ERR_INVALID.
 */
#define PYG_HIP_MM_SCHED_AUTO 0
#define PYG_HIP_MM_SCHED_CONTIGUOUS 1
#define PYG_HIP_MM_SCHED_CYCLIC 2
#define PYG_HIP_MM_SCHED_TICKET 3
#define PYG_HIP_MM_SCHED_GENERAL 4
#define PYG_HIP_MM_SCHED_NAIVE 5
#define PYG_HIP_MM_SCHED_RING 6
#define PYG_HIP_MM_SCHED_MASK 0xf
#define PYG_HIP_MM_F32_SPLIT 0x100

/* Workspace (device bytes) needed by pyg_hip_segment_matmul / pyg_hip_grouped_matmul for
 * `num_groups` segments/groups. */
PYG_HIP_API size_t pyg_hip_matmul_workspace_size(int64_t num_groups);

/*
 * out[ptr[b]:ptr[b+1]] = input[ptr[b]:ptr[b+1]] @ other[b]            for b in [0, B)
 * Replaces pyg::segment_matmul (schema pyg_lib/csrc/ops/matmul.cpp:66-67; CPU kernel
 * pyg_lib/csrc/ops/cpu/matmul_kernel.cpp:410-439; CUDA kernel
 * pyg_lib/csrc/ops/cuda/matmul_kernel.cu:304-319).
 *   input  [N, K] row-major, other [B, K, M] row-major, out [N, M] row-major, all `dtype`.
 *   ptr    B+1 int64 boundaries; on device if ptr_on_device != 0, else on the host (the
 *          reference's preferred placement, pyg_lib/ops/__init__.py:160-161).  Unlike the
 *          reference no host synchronisation happens in either case.
 *   bias   optional [B, M] (may be NULL): fused epilogue for the Python-side loop
 *          pyg_lib/ops/__init__.py:169-171.
 *   flags  PYG_HIP_MM_* above (0 = automatic schedule, exact fp32).
 *   Rows outside [ptr[0], ptr[B]) are left untouched (the reference leaves them
 *   uninitialised, matmul_kernel.cpp:416).
 */
PYG_HIP_API int pyg_hip_segment_matmul(int dtype, const void* input, const int64_t* ptr,
                                       int ptr_on_device, const void* other, const void* bias,
                                       void* out, int64_t N, int64_t K, int64_t M, int64_t B,
                                       void* workspace, size_t workspace_bytes, int flags, void* stream);

/* One group of a grouped matmul: out[rows, m] = input[rows, k] @ other[k, m].
 * `other_trans` != 0 means `other` is stored [m, k] row-major (a transposed view, as produced
 * by the backward pass pyg_lib/ops/__init__.py:84,91), read in place. */
typedef struct {
  const void* input;
  const void* other;
  void* out;
  int64_t rows;
  int32_t k;
  int32_t m;
  int32_t other_trans;
  int32_t reserved;
} pyg_hip_group;

/*
 * outs[i] = inputs[i] @ others[i] for i in [0, G).
 * Replaces pyg::grouped_matmul (schema pyg_lib/csrc/ops/matmul.cpp:64-65; CPU kernel
 * pyg_lib/csrc/ops/cpu/matmul_kernel.cpp:281-312; CUDA kernel
 * pyg_lib/csrc/ops/cuda/matmul_kernel.cu:289-302).  `groups_host` is a HOST array of G
 * descriptors (copied asynchronously into the workspace).
 */
PYG_HIP_API int pyg_hip_grouped_matmul(int dtype, const pyg_hip_group* groups_host, int64_t G,
                                       void* workspace, size_t workspace_bytes, int flags, void* stream);

/* Name of the kernel variant the last matmul call on this thread dispatched to
 * ("mfma_bf16_k128_m128", "naive", ...): lets tests assert that the MFMA path ran. */
PYG_HIP_API const char* pyg_hip_matmul_last_variant(void);

/*
 * Weight gradient of segment_matmul:  grad_other[b] = input[ptr[b]:ptr[b+1]]^T @ grad_out[ptr[b]:ptr[b+1]]
 * (input [N, K], grad_out [N, M], grad_other [B, K, M]; fp32 accumulation, one rounding).  Replaces the
 * per-relation loop of SegmentMatmul::backward (ops/autograd/matmul_kernel.cpp:92-107: B x
 * at::matmul(input_i^T, grad_out_i) + at::stack) with one persistent launch.  fp32 / bf16 / fp16, ANY K and M and any
 * element-aligned operands; which kernel runs is the table of pyg_hip_matmul_dw_route below.  fp32 multiplies on
 * v_mfma_f32_32x32x2_f32 (IEEE fp32).  Other dtypes return PYG_HIP_ERR_UNSUPPORTED (the caller keeps the reference formula).
 *   ptr        B+1 int64 boundaries, on device if ptr_on_device != 0; a host `ptr` must be non-decreasing within [0, N]
 *              (PYG_HIP_ERR_INVALID before anything is launched), a device `ptr` is trusted.
 *   workspace  pyg_hip_segment_matmul_dw_workspace_size(B, K, M) bytes of device scratch (tile plan + fp32 partial slabs).
 * Checks, in this order: an empty call (B x K x M == 0) returns at once; NULL tensors; dtype; workspace; operands that
 * are not element-aligned (PYG_HIP_ERR_INVALID); a shape beyond the general kernel (PYG_HIP_ERR_UNSUPPORTED); 2^31 or
 * more work tiles (PYG_HIP_ERR_INVALID).  Never synchronises.
 */
PYG_HIP_API size_t pyg_hip_segment_matmul_dw_workspace_size(int64_t B, int64_t K, int64_t M);
/* Grouped form (the others_grad of GroupedMatmul.backward, pyg_lib/ops/__init__.py:88-94): for every
 * group i, out_i = input_i^T @ other_i with input_i [rows_i, k_i] and other_i [rows_i, m_i] row-major, PER-GROUP k_i,
 * m_i (`out` / `other_trans` of pyg_hip_group are ignored); out_pool receives the [k_i, m_i] results back to back in
 * group order (out_i starts at element sum_{j < i} k_j m_j; uniform shapes: one [G, k, m] block).  Workspace:
 * pyg_hip_grouped_matmul_dw_workspace_size(groups, G). */
PYG_HIP_API size_t pyg_hip_grouped_matmul_dw_workspace_size(const pyg_hip_group* groups, int64_t G);
/*
 * The route of a weight-gradient call, as a name; launches nothing, touches no device, keeps no state (the returned string
 * lives in a thread-local buffer until the next query on the thread).  Both entry points take the route this answers.
 *   uniform   != 0: all groups share (K, M) -- always so for the segment form
 *   misalign  the low four address bits of every X and dY operand of the call, ORed together, plus the bits of the
 *             output address below the element size (dW is stored element by element: the output only has to be
 *             element-aligned)
 * The first line that applies:
 *   unsupported           dtype not f32 / bf16 / f16
 *   invalid               misalign % element size != 0 (or K, M < 0)
 *   gen                   not uniform, or misalign % 16 != 0, or not (K in {64, 128, 256} and M > 0 and M % 64 == 0): the
 *                         general-shape kernel (matmul_dw_gen.hip: 128 x 128 output blocks, fp32 128 x 64, tails
 *                         zero-filled in LDS, widest vector loads the alignment allows) -- but
 *   unsupported           for such a call with K >= 2^21, M >= 2^21 or K x M >= 2^28 (the kernel's 32-bit offsets)
 *   wide256_<bf16|f16>    16-bit, K = 256, M % 256 == 0: 256 output columns per workgroup, the waves split the columns
 *   seg_<t>_k<K>_mc<MC>   everything else, t = bf16 | f16 | f32: every wave owns a K x MC accumulator block, M / MC column
 *                         chunks per tile range;  K = 64, 128: MC = 128 if M % 128 == 0, else 64;  K = 256: MC = 64
 *                         (fp32 K = 256 also when M % 256 == 0)
 */
PYG_HIP_API const char* pyg_hip_matmul_dw_route(int dtype, int64_t K, int64_t M, int uniform, unsigned misalign);
/* Diagnostic: calls served by the shape-specialised (seg_*, wide256_*) / the general-shape (gen) weight-gradient kernels
 * since the library was loaded (process wide); a call counts once it has returned PYG_HIP_OK.  Either pointer may be NULL. */
PYG_HIP_API void pyg_hip_matmul_dw_counters(int64_t* specialised, int64_t* general);
PYG_HIP_API int pyg_hip_grouped_matmul_dw(int dtype, const pyg_hip_group* groups, int64_t G, void* out_pool,
                                          void* workspace, size_t workspace_bytes, void* stream);
PYG_HIP_API int pyg_hip_segment_matmul_dw(int dtype, const void* input, const int64_t* ptr, int ptr_on_device,
                                          const void* grad_out, void* grad_other, int64_t N, int64_t K,
                                          int64_t M, int64_t B, void* workspace, size_t workspace_bytes,
                                          void* stream);

/* ---- fused relational graph convolution (BASELINE config C5) -------------- */

/* One relation of pyg_hip_rgcn_fused: its sampled edges e in [0, num_edges) read row
 * gather_index[e] + gather_offset of x and add their message to row scatter_index[e] + scatter_offset of out.
 * The index vectors are the per-relation `col` / `row` outputs of hetero_neighbor_sample, used in place. */
typedef struct {
  const int64_t* gather_index;  /* device */
  const int64_t* scatter_index; /* device; runs of equal values are summed before they touch memory */
  int64_t num_edges;
  int64_t gather_offset;
  int64_t scatter_offset;
  const void* weight;           /* device, [K, M] row-major, 16-byte aligned */
  /* Optional second indirection ("true fusion": the per-batch feature matrix x is never materialised).  With `x`
   * non-NULL this relation gathers from its OWN table x [x_rows, K] (e.g. the global feature table of its source
   * node type) at row gather_map[gather_index[e]] (gather_map = that type's sampled node ids, gather_map_len
   * entries), or gather_index[e] + gather_offset if gather_map is NULL.  All zero: the call's x, as before. */
  const void* x;
  const int64_t* gather_map;
  int64_t x_rows;
  int64_t gather_map_len;
  /* Rows of `out` this relation may write: [scatter_offset, scatter_offset + scatter_rows) -- the row count of its
   * destination node type (the `dim_size` of the reference's reductions, pyg_lib/csrc/ops/scatter.cpp:156-160).  0: up to
   * num_out_rows.  PYG_HIP_RGCN_GROUPED validates scatter_index against it (error 2) and sizes its row-start workspace by
   * it (sum of scatter_rows over the relations instead of R x num_out_rows); the atomic kernel validates against
   * num_out_rows only. */
  int64_t scatter_rows;
} pyg_hip_rgcn_relation;

PYG_HIP_API size_t pyg_hip_rgcn_fused_workspace_size(int64_t num_relations, int64_t num_edges);

/*
 * out[scatter_index_r[e] + scatter_offset_r] += x[gather_index_r[e] + gather_offset_r] @ weight_r  for all r, e.
 * One launch replacing the chain gather_coo -> segment_matmul -> scatter_sum of the reference ops
 * (pyg_lib/csrc/ops/cuda/segment_coo_kernel.cu:1316-1360, ops/cuda/matmul_kernel.cu:304-319,
 * ops/cuda/scatter_kernel.cu:56-71): the gathered rows and the messages never exist in HBM.
 *   x [num_x_rows, K], out [num_out_rows, M] (ACCUMULATED into: zero it for a plain aggregation), both `dtype`
 *   row-major; which types and shapes are served: the table of pyg_hip_rgcn_route below (others:
 *   PYG_HIP_ERR_UNSUPPORTED, the caller keeps the three-op chain).  Messages are rounded to `dtype` once (as the chain does), runs of equal destination are
 *   summed in fp32 and added with packed 16-bit atomics.  `relations` is a host array.  `checked` is a bit field
 *   (PYG_HIP_RGCN_*): PYG_HIP_RGCN_CAS makes the packed adds compare-and-swap loops (see pyg_hip_set_float_atomic_mode).
 *   Never synchronises -- unless PYG_HIP_RGCN_CHECKED is set: then every gather / scatter index is validated against num_x_rows (x_rows, gather_map_len)
 *   / num_out_rows on the device, offenders are redirected to row 0, and the call waits for the stream and returns
 *   PYG_HIP_ERR_INVALID if there was one (unchecked, a bad index is an out-of-bounds read / an atomic into foreign memory).
 */
#define PYG_HIP_RGCN_CHECKED 1
#define PYG_HIP_RGCN_CAS 2
#define PYG_HIP_RGCN_DEFERRED 4
/* PYG_HIP_RGCN_DEFERRED (ignored with _CHECKED): the same validation WITHOUT the synchronisation -- offenders are
 * redirected to row 0, so a stale node id is never an out-of-bounds access, and the kernel leaves 1 (gather) / 2
 * (scatter) / 3 (not grouped, PYG_HIP_RGCN_GROUPED) in a pinned word of the device.  The next pyg_hip_rgcn_fused call with this flag on that device fails with
 * PYG_HIP_ERR_INVALID naming the earlier call; pyg_hip_rgcn_pending_error() returns and clears the word (meaningful once
 * the stream has been synchronised).  This is what the torch binding passes by default (PYG_HIP_RGCN_CHECK=1: _CHECKED,
 * =0: no validation). */
PYG_HIP_API int pyg_hip_rgcn_pending_error(void);
/* PYG_HIP_RGCN_GROUPED: the caller promises that every relation's scatter_index is NONDECREASING (edges grouped by
 * destination -- what the neighbour samplers emit: `row` of every edge type, csc = false).  Then no atomics are needed:
 * a small launch finds every destination's first edge, and an owner-computes kernel (32 rows of `out` per workgroup)
 * sums every row's source features in fp32 in edge order, multiplies the 32 sums of a relation with its weight in one
 * MFMA tile, accumulates the relations of a row in fp32 and WRITES every row of `out` once (rows without edges: zeros).
 *   - `out` is OVERWRITTEN, not accumulated into (do not zero it); it must be 16-byte aligned;
 *   - more types and shapes than the atomic kernel's (the table of pyg_hip_rgcn_route below): the feature rows are walked
 *     per 128-feature slice, W travels through LDS in 128 x 128 chunks;
 *   - the same bits on every run; rounding: the per-relation feature sum and the result are each rounded once;
 *   - the workspace is pyg_hip_rgcn_grouped_workspace_size() bytes (4 bytes per row of every relation's destination
 *     segment -- scatter_rows, or the rows of `out` at and behind its scatter_offset if that is 0: row starts, touched
 *     only where edges arrive);
 *   - fewer than 2^31 rows of `out` and edges per relation (PYG_HIP_ERR_UNSUPPORTED otherwise);
 *   - with _CHECKED / _DEFERRED the promise is verified on the device: a descent in a scatter_index is error 3
 *     (PYG_HIP_ERR_INVALID "not grouped"; the result of such a call is unspecified but every access stays in bounds),
 *     an out-of-range scatter index drops its edge (error 2), a gather index is redirected to row 0 (error 1). */
#define PYG_HIP_RGCN_GROUPED 8
PYG_HIP_API size_t pyg_hip_rgcn_grouped_workspace_size(const pyg_hip_rgcn_relation* relations, int64_t num_relations,
                                                       int64_t num_out_rows);
PYG_HIP_API int pyg_hip_rgcn_fused(int dtype, const void* x, int64_t num_x_rows, const pyg_hip_rgcn_relation* relations,
                                   int64_t num_relations, void* out, int64_t num_out_rows, int64_t K, int64_t M,
                                   int checked, void* workspace, size_t workspace_bytes, void* stream);
/*
 * Which kernel family serves a call.  pyg_hip_rgcn_route(dtype, K, M, num_relations, flags) answers without touching a device
 * (`flags`: the `checked` bit field; only PYG_HIP_RGCN_GROUPED matters).  The first row that applies:
 *
 *   flags      dtype        K, M                                          route
 *   any        any          num_relations < 0 or >= 2^30                  unsupported
 *   GROUPED    any          num_relations > 512                           unsupported
 *   -          bf16, f16    128 x 128                                     atomic             packed 16-bit atomic adds
 *   -          anything else                                              unsupported
 *   GROUPED    bf16, f16    128 x 128                                     grouped_128        the four-deep item pipeline
 *   GROUPED    bf16, f16    128 x 256, 256 x 128, 256 x 256               grouped_shape      the pipeline over 128-feature sub-items
 *   GROUPED    bf16, f16    other multiples of 8 in [8, 256]              grouped_small      run-time row sizes, item at a time
 *   GROUPED    f32          128 x 128                                     grouped_f32        fp32 sums, fp32 MFMAs
 *   GROUPED    f32          other multiples of 4 in [4, 128]              grouped_f32_small  run-time row sizes, FMAs
 *   GROUPED    anything else                                              unsupported
 *
 * pyg_hip_rgcn_fused refuses an unsupported call (PYG_HIP_ERR_UNSUPPORTED; a dtype no row names: PYG_HIP_ERR_INVALID).  What a
 * route does not decide follows from the call: with up to 24 relations their records travel in the kernel argument (`inline`),
 * longer lists are staged through the workspace (`staged`); a feature table of 4 GB or more takes the instances with 64-bit row
 * offsets (`big`); PYG_HIP_RGCN_CHECKED / _DEFERRED select the validating instances of atomic and grouped_128 (`check`; the
 * other families always validate and report only with one of the two flags).
 * pyg_hip_rgcn_last_route() names the last launch of the calling thread:
 *   "<route> kc<KC> mc<MC> <bf16|f16|f32> <check|nocheck> <big|nobig> <inline|staged>"
 * (KC, MC: the 128-feature slices of a feature row / a row of `out` the kernel is instantiated for), "none" before the first
 * one; a call that launches nothing (no relations, no edges) leaves it as it is.
 */
#define PYG_HIP_RGCN_ROUTE_UNSUPPORTED 0
#define PYG_HIP_RGCN_ROUTE_ATOMIC 1
#define PYG_HIP_RGCN_ROUTE_GROUPED_128 2
#define PYG_HIP_RGCN_ROUTE_GROUPED_SHAPE 3
#define PYG_HIP_RGCN_ROUTE_GROUPED_SMALL 4
#define PYG_HIP_RGCN_ROUTE_GROUPED_F32 5
#define PYG_HIP_RGCN_ROUTE_GROUPED_F32_SMALL 6
PYG_HIP_API int pyg_hip_rgcn_route(int dtype, int64_t K, int64_t M, int64_t num_relations, int flags);
PYG_HIP_API const char* pyg_hip_rgcn_last_route(void);

/* ---- neighbor_sample / hetero_neighbor_sample ---------------------------------------------- */

/* Host services the sampler needs from its caller (the torch binding supplies the PyTorch
 * caching allocator and the global CPU generator, so device memory and torch.manual_seed()
 * behave exactly as for the reference operator). */
/* State of an at::mt19937 engine (ATen/core/MT19937RNGEngine.h: state_[624], left_, next_). */
typedef struct {
  uint32_t state[624];
  int32_t left;
  uint32_t next;
} pyg_hip_mt19937;

typedef struct {
  void* user;
  /* Device allocation on the stream the sampler runs on; NULL on failure. */
  void* (*alloc)(void* user, size_t bytes);
  /* Release a block obtained from `alloc` (stream-ordered with the sampler's stream). */
  void (*free)(void* user, void* ptr);
  /* Fill num_blocks x 128 host int64 words exactly like that many consecutive RandintEngine
   * prefetches (pyg_lib/csrc/random/cpu/rand_engine.h:79-91): the first prefetch of a call is
   * at::randint(INT64_MIN, INT64_MAX, {128}) (first != 0), later ones are in-place
   * random_(INT64_MIN, INT64_MAX) refills.  Both draw the same serial mt19937 stream, so one
   * random_ over num_blocks*128 elements is equivalent. */
  void (*rng_blocks)(void* user, int64_t* words_host, int64_t num_blocks, int first);
  /* Optional fast path: the state of the CPU generator's mt19937 engine (in/out, host memory).  If
   * non-NULL the words are generated ON THE DEVICE by continuing this engine exactly as random_
   * would (two 32-bit outputs per word, high half first, % (2^64-1) + INT64_MIN), rng_blocks is not
   * called, and the advanced state is written back before the call returns. */
  pyg_hip_mt19937* mt19937;
} pyg_hip_sampler_host;

/* One CSR relation of a (heterogeneous) graph.  src_type / dst_type index `node_types` in the
 * order the reference's `edge_types` tuples name them (roles swap when csc, neighbor_kernel.cpp
 * :715-716). */
typedef struct {
  const int64_t* rowptr; /* device, num_rows + 1 */
  int64_t num_rows;
  const int64_t* col;    /* device */
  int64_t num_cols;
  int32_t src_type;
  int32_t dst_type;
  const int64_t* num_neighbors_host; /* L fan-outs, host */
  const int64_t* edge_time;          /* device, per edge, or NULL (edge-level temporal sampling) */
  /* Biased sampling (neighbor_kernel.cpp:39-56,245-285; hetero :732-745): per-edge weights on the device, or
   * NULL.  edge_weight_dtype is PYG_F32 or PYG_F64 (the dtype decides how many generator outputs a draw
   * takes, see pyg_hip_hetero_neighbor_sample).  Needs host->mt19937. */
  const void* edge_weight;
  int32_t edge_weight_dtype;
  /* != 0: rowptr and col point at int32 arrays (declared int64_t* for source compatibility) and are read in
   * place; the reference's int32 instantiation (neighbor_kernel.cpp:893,930).  Seeds, times and all outputs stay
   * int64 on this interface (they are a few thousand to a million elements; the binding converts them). */
  int32_t index_is32;
} pyg_hip_relation;

/* Seeds of one node type, in seed_dict iteration order. */
typedef struct {
  int32_t node_type;
  int32_t reserved;
  const int64_t* seed; /* device */
  int64_t num_seed;
  const int64_t* seed_time; /* device, per seed, or NULL (then node_time[seed] is used) */
} pyg_hip_seed_set;

/* Results.  All pointers come from host->alloc and are owned by the caller afterwards (blocks
 * may be larger than the element counts given here).
 *   per node type t:  node_id[t] -> num_nodes[t] ids ([n] int64, or [n, 2] (batch, node) pairs
 *                     when disjoint), nodes_per_hop_host[t*(L+1) ..]
 *   per relation e:   row[e], col[e], edge_id[e] (NULL unless return_edge_id) -> num_edges[e],
 *                     edges_per_hop_host[e*L ..]
 * The `*_host` arrays and the pointer arrays are caller-provided host memory. */
typedef struct {
  int64_t** node_id;
  int64_t* num_nodes;
  int64_t* nodes_per_hop_host;
  int64_t** row;
  int64_t** col;
  int64_t** edge_id;
  int64_t* num_edges;
  int64_t* edges_per_hop_host;
  int64_t rng_blocks; /* 128-word prefetches consumed (incl. the constructor's) */
} pyg_hip_sample_result;

/*
 * Multi-hop neighbour sampling with first-occurrence-ordered node relabelling, bit-exact with
 * the reference's single-threaded CPU kernel (pyg_lib/csrc/sampler/cpu/neighbor_kernel.cpp
 * :518-841; homogeneous :332-514 is the 1-type / 1-relation case; schemas
 * pyg_lib/csrc/sampler/neighbor.cpp:130-147).  The reference has no device sampler at all.
 *
 * flags: csc, replace, disjoint, return_edge_id as in the schema.  `directed` must be true
 * (the reference errors otherwise, neighbor_kernel.cpp:501).
 * Temporal sampling (node_temporal_sample / edge_temporal_sample, neighbor_kernel.cpp:74-144;
 * requires disjoint): node_time_by_type is a host array of num_node_types device pointers (entries
 * or the array itself may be NULL), relation.edge_time takes precedence; temporal_last selects the
 * "last" strategy.  A neighbourhood that is not time-sorted fails with the reference's message.
 * Biased sampling (relation.edge_weight; _biased_sample, neighbor_kernel.cpp:245-285): a row with more
 * neighbours than the fan-out draws one uniform number per neighbour STRAIGHT from the generator (one
 * 32-bit output per float32 weight, 24 bits kept; two per float64 weight, 53 bits kept -- Tensor.uniform_),
 * key = log(u) / weight, and takes the `count` largest keys in Tensor.topk order (ties as libstdc++'s
 * partial_sort / nth_element + sort leave them, ATen/native/TopKImpl.h).  The device path reproduces that
 * stream and that order; `log` is the correctly rounded logarithm where libtorch calls MKL's (<1 ulp, closed
 * source: 15,372 of the 2^24 possible float32 arguments round differently), so a selection can differ from
 * the reference's only if two keys of one row lie within one ulp of each other.  Weighted and unweighted
 * relations may be mixed (the engine's later 128-word blocks then lie behind the weighted relations' draws in
 * the generator stream, as in the reference).  With replace != 0 the reference calls
 * at::multinomial(weight, count, true): for count > 1 that is a sequential cumulative sum in the weights' type,
 * a division by the sum, and one 53-bit double per sample located by binary search -- reproduced exactly
 * (PYG_HIP_ERR_INVALID "invalid multinomial distribution" for rows at::multinomial rejects); for count == 1
 * at::multinomial takes argmax(weight / exponential_()) instead, where libtorch 2.10 draws one 53-bit double
 * per neighbour and evaluates -log1p(-u) -- reproduced too (first of equal maxima).  Temporal arguments and a
 * missing host->mt19937 fail with PYG_HIP_ERR_UNSUPPORTED.
 * Synchronises `stream` (output sizes are data dependent).
 */
/* Driver the calling thread's last neighbor / hetero sampler call ran: "fused" (bounded fan-outs <= 1024: 2 - 3 launches
 * per hop -- scans of up to 256 tiles are one launch, PYG_HIP_SAMPLER_ONEPASS=0: always a reduce + apply pair --,
 * csrc/hip/sampler_fused.h; since round 5 also with rows of degree >= 2^16, whose 32-bit draws the chain's transition
 * tables carry, and with fan-outs above 64, sampled one wave per node), "queued" (round 2's chain:
 * PYG_HIP_SAMPLER_FUSED=0 or more than 3 relations expanding one node type; fan-outs <= 64), "synchronising"
 * (unbounded / > 1024 fan-outs, weighted relations, more wide draws than the speculated random words allow, or
 * PYG_HIP_SAMPLER_SYNC_MODE=1).  Diagnostics only; every driver returns the same bits. */
PYG_HIP_API const char* pyg_hip_sampler_last_mode(void);
/* Direct-address node tables of the fused chain are kept between calls (per device and node count; blocks come from
 * host->alloc and are never freed): a call's values carry an epoch in their upper bits, so what an earlier call left
 * behind reads as "empty" and the 19.6 MB clear of a products-sized table (one launch, 7 % of a batch's traffic; four
 * launches for the MAG-shaped C5 graph) happens once per 2^20 - 1 calls instead of every call.  Diagnostics / tests:
 * `limit` = epochs per clear (0: the default 2^20 - 1); returns the number of tables cached for the current device.
 * PYG_HIP_SAMPLER_TABLE_CACHE=0 disables the cache (every call clears a fresh table, as before round 4). */
PYG_HIP_API int pyg_hip_sampler_table_cache(int64_t limit);
/* Frees the cached tables of the current device that no call is using, through host->free (the allocator they came
 * from); returns how many stay (busy ones).  The cache holds at most 8 tables of <= 128 MiB per device; an idle table
 * of another node count is evicted when a new size needs room. */
PYG_HIP_API int pyg_hip_sampler_table_cache_release(const pyg_hip_sampler_host* host);
/*
 * The random-word stream kept between calls.  A data loader samples batch after batch on ONE generator
 * (benchmark/sampler/neighbor.py:101-121 seeds once per run): the engine a call hands back through host->mt19937 is the
 * engine the next call presents, and the words the library generated beyond a call's own consumption are exactly the next
 * call's words.  The fused chain keeps them per device (buffer of <= 64 MiB from host->alloc, the handed-back engine) and
 * adopts them when the presented engine equals the kept one bit for bit: then no generation launch and no cross-stream
 * wait lies in front of any hop, and the next round is generated in the background, two calls' worth ahead.  Any other
 * engine (reseeded, used elsewhere in between) misses and the call starts cold -- same bits either way, the generator
 * ends where the reference's engine leaves it.  PYG_HIP_SAMPLER_RNG_CARRY=0 disables it;
 * pyg_hip_sampler_table_cache_release also frees the idle stream.  Counters since process start: calls that adopted a
 * kept stream / calls that looked for one and started cold.
 */
PYG_HIP_API int pyg_hip_sampler_rng_carry_stats(int64_t* adopted, int64_t* cold);

PYG_HIP_API int pyg_hip_hetero_neighbor_sample(int num_node_types, int num_relations,
                                               const pyg_hip_relation* relations_host,
                                               int num_seed_sets,
                                               const pyg_hip_seed_set* seeds_host,
                                               const int64_t* const* node_time_by_type,
                                               int temporal_last, int L, int csc, int replace,
                                               int disjoint, int return_edge_id,
                                               const pyg_hip_sampler_host* host,
                                               pyg_hip_sample_result* result, void* stream);

/*
 * K independent sampler calls on one graph at once (the epoch loop of the reference's benchmark,
 * benchmark/sampler/neighbor.py:101-121, handed over as a whole; semantics per batch: sampler/cpu/neighbor_kernel.cpp
 * :332-514 / :518-841).  Batch b = its own seed sets, its own `host` (allocator context + generator state: every batch
 * continues ITS OWN mt19937 stream -- torch.manual_seed(s_b) per batch is the reference benchmark's protocol) and its own
 * result; everything else is shared.  Results are bit for bit those of pyg_hip_hetero_neighbor_sample on each batch alone.
 * Batches that name different `stream`s are driven by different host threads of a persistent pool inside the library and
 * overlap on the device (a single batch is a chain of ~12 small dependent launches that cannot fill 256 CUs); batches on the
 * same stream run one after the other.  host->alloc of a batch must allocate for THAT batch's stream.  `stream` = the
 * caller's stream: work queued on it before the call is ordered in front of every batch; all batches are complete (their
 * streams synchronised) when the call returns.  Returns the first failing batch's status; `status` / `error` / `mode`
 * (pyg_hip_sampler_last_mode of that batch) are filled per batch.
 */
typedef struct {
  int num_seed_sets;
  const pyg_hip_seed_set* seeds_host;
  const pyg_hip_sampler_host* host;
  pyg_hip_sample_result* result;
  void* stream;
  int status;         /* out */
  const char* mode;   /* out */
  char error[256];    /* out */
} pyg_hip_sample_batch;
PYG_HIP_API int pyg_hip_hetero_neighbor_sample_batched(int num_node_types, int num_relations,
                                                       const pyg_hip_relation* relations_host,
                                                       const int64_t* const* node_time_by_type, int temporal_last,
                                                       int L, int csc, int replace, int disjoint, int return_edge_id,
                                                       int num_batches, pyg_hip_sample_batch* batches, void* stream);

/*
 * The float32 logarithm biased sampling evaluates (key = log(u) / weight), element-wise over device arrays.
 * Exposed so that it can be pinned on every argument Tensor.uniform_ can produce (k * 2^-24).
 */
PYG_HIP_API int pyg_hip_biased_log_f32(const float* in, float* out, int64_t n, void* stream);

/*
 * One-hop sampling WITHOUT relabelling for PyG's distributed sampler.
 * Replaces pyg::dist_neighbor_sample (schema pyg_lib/csrc/sampler/neighbor.cpp:148-153; CPU kernel
 * sampler/cpu/neighbor_kernel.cpp:957-978, `distributed` flag :296-303,386-388,446-447).
 *   node_id   -> S + E ids (seeds first, then every sampled destination, duplicates kept;
 *                [S+E, 2] (batch, node) pairs when disjoint), from host->alloc
 *   edge_id   -> E sampled edge ids, from host->alloc
 *   cumsum_host  caller array of S + 1 entries: [S, size after seed 0, size after seed 1, ...]
 * Random words, temporal arguments, biased sampling (edge_weight: device pointer or NULL, edge_weight_dtype
 * PYG_F32 / PYG_F64) and error behaviour as in pyg_hip_hetero_neighbor_sample.  index_is32 != 0: rowptr and col point at
 * int32 arrays and are read in place (the reference's int32 instantiation, neighbor_kernel.cpp:893); seeds, times and the
 * outputs stay int64 on this interface.
 */
PYG_HIP_API int pyg_hip_dist_neighbor_sample(const int64_t* rowptr, const int64_t* col,
                                             const int64_t* seed, int64_t num_seed,
                                             int64_t num_neighbors, const int64_t* node_time,
                                             const int64_t* edge_time, const int64_t* seed_time,
                                             const void* edge_weight, int edge_weight_dtype,
                                             int temporal_last, int replace, int disjoint, int index_is32,
                                             const pyg_hip_sampler_host* host, int64_t** node_id,
                                             int64_t** edge_id, int64_t* num_edges,
                                             int64_t* cumsum_host, void* stream);

/*
 * Building blocks of pyg::hetero_relabel_neighborhood (schema sampler/dist_relabel.cpp:77-83; CPU
 * sampler/cpu/dist_relabel_kernel.cpp:96-262): there every node type has ONE Mapper and consumes its
 * `sampled_nodes_with_duplicates` list strictly in order, so the local id of list position j is a per-type
 * quantity (pyg_hip_relabel_nodes), and an edge type's rows / cols are segments of source indices
 * (pyg_hip_expand_rows) / of the destination type's local ids.
 *   pyg_hip_relabel_nodes: local_out[j] = Mapper id of sampled[j] after the seeds (ids of first occurrences;
 *     disjoint: keys (batch, node), the seeds carry batch ids seed_batch0, seed_batch0 + 1, ..., all batch ids
 *     < num_batches).  Workspace: pyg_hip_relabel_workspace_size(num_seed, num_sampled).
 *   pyg_hip_expand_rows: row_out[j] = i for count_prefix[i] <= j < count_prefix[i + 1] (device prefix of
 *     num_src + 1 entries), j < total.
 */
PYG_HIP_API int pyg_hip_relabel_nodes(const int64_t* seed, int64_t num_seed, int64_t seed_batch0,
                                      int64_t num_batches, const int64_t* sampled, int64_t num_sampled,
                                      const int64_t* batch, int disjoint, int64_t* local_out,
                                      void* workspace, size_t workspace_bytes, void* stream);
PYG_HIP_API int pyg_hip_expand_rows(const int64_t* count_prefix, int64_t num_src, int64_t total,
                                    int64_t* row_out, void* stream);

/*
 * Distributed-sampling helpers (homogeneous forms).
 *
 * pyg_hip_relabel_neighborhood replaces pyg::relabel_neighborhood (schema sampler/dist_relabel.cpp:71-76; CPU
 * sampler/cpu/dist_relabel_kernel.cpp:30-94): local ids in insertion order -- the seeds first (a duplicate
 * seed keeps the id of its first occurrence; disjoint: key (i, seed[i])), then the externally sampled
 * sequence `sampled` (disjoint: key (batch[j], sampled[j])).  col_out[j] = id of sampled[j]; row_out[j] = the
 * source node i with count_prefix[i] <= j < count_prefix[i + 1] (count_prefix: device array of num_src + 1
 * offsets, the running sum of num_sampled_neighbors_per_node).  The csc swap is the caller's.
 * `workspace`: pyg_hip_relabel_workspace_size(num_seed, num_sampled) bytes.
 *
 * pyg_hip_segment_concat is the device part of pyg::merge_sampler_outputs (schema
 * sampler/dist_merge_outputs.cpp:51-55; CPU sampler/cpu/dist_merge_outputs_kernel.cpp:17-138): out = the
 * segments bases[part[j]][begin[j] ...) of length dst_off[j+1] - dst_off[j], concatenated in j order; with
 * `fill`, out[i] = fill[j] for the positions of segment j instead (the batch vector).  All arrays are device
 * arrays; `bases` is a device array of device pointers.
 */
PYG_HIP_API size_t pyg_hip_relabel_workspace_size(int64_t num_seed, int64_t num_sampled);
PYG_HIP_API int pyg_hip_relabel_neighborhood(const int64_t* seed, int64_t num_seed, const int64_t* sampled,
                                             int64_t num_sampled, const int64_t* count_prefix, int64_t num_src,
                                             const int64_t* batch, int disjoint, int64_t* row_out, int64_t* col_out,
                                             void* workspace, size_t workspace_bytes, void* stream);
PYG_HIP_API int pyg_hip_segment_concat(const int64_t* const* bases, const int64_t* part, const int64_t* begin,
                                       const int64_t* dst_off, int64_t n, const int64_t* fill, int64_t* out,
                                       int64_t total, void* stream);

/* ---- random_walk / subgraph ---------------------------------------------------------------- */

/*
 * Uniform random walks.  Replaces pyg::random_walk (schema pyg_lib/csrc/sampler/random_walk.cpp:29-32; CUDA kernel
 * sampler/cuda/random_walk_kernel.cu:27-88).  index_dtype is PYG_I32 or PYG_I64 and types rowptr (num_nodes + 1),
 * col (num_edges), seed (num_seeds) and out ([num_seeds, walk_length + 1], row-major, seeds in column 0).
 * `rand` holds walk_length x num_seeds float32 uniforms in [0, 1) (the caller draws them as the reference does:
 * at::rand({walk_length, num_seeds}) on the seeds' device); step j of walk i uses rand[j * num_seeds + i]:
 * v <- col[rowptr[v] + min(trunc(float(u) * float(deg)), deg - 1)] when deg = rowptr[v + 1] - rowptr[v] > 0, else v
 * stays (the reference's "fake self-loop").  A node outside [0, num_nodes) -- a seed or a col entry -- and a row whose
 * rowptr pair leaves [0, num_edges] are treated as isolated: nothing outside rowptr / col is read (the reference's
 * behaviour there is undefined).  walk_length < 0 fails with PYG_HIP_ERR_INVALID.  Does not synchronise.
 * A block's output tile is written through LDS (16-byte stores) where it fits in 64 KiB; PYG_HIP_WALK_STAGE=0 writes
 * every step straight from registers instead (A/B switch).
 */
PYG_HIP_API int pyg_hip_random_walk(int index_dtype, const void* rowptr, int64_t num_nodes, const void* col,
                                    int64_t num_edges, const void* seed, int64_t num_seeds, const float* rand,
                                    int64_t walk_length, void* out, void* stream);

/*
 * node2vec walks: second-order random walks with return parameter p and in-out parameter q (this build only; the
 * reference's pyg::random_walk stops at p = q = 1).  Buffers and the treatment of nodes outside the graph are those of
 * pyg_hip_random_walk.  The result is a pure function of the arguments: the same on the device, on the binding's CPU key
 * and in tests/_node2vec_ref.py, bit for bit.  One lane per walk; no atomics, no allocation, no synchronisation.
 *
 * Word stream.  Walk i is the i-th seed.  Its stream of 32-bit words is the successive results of
 * at::Philox4_32(key, subsequence = i, offset = 0)::operator() (ATen/core/PhiloxRNGEngine.h): Philox4x32-10 with key = the
 * two halves of `key`, counter = (n_lo, n_hi, i_lo, i_hi) for the n-th block of four words, outputs consumed in index
 * order 0..3.
 * Uniform.  A word becomes u = float(word >> 8) * 2^-24, in [0, 1).
 * Thresholds.  The caller computes them once in double and rounds to float32: M = max(1/p, 1, 1/q), a_ret = (1/p)/M,
 * a_near = 1/M, a_far = (1/q)/M.  Each must lie in (0, 1] (else PYG_HIP_ERR_INVALID).
 * Stays.  A current node v outside [0, num_nodes), or whose rowptr pair is empty or leaves [0, num_edges], makes the walk
 * stay and consumes no words.
 * Step 1 (no predecessor).  One word: v1 = col[rs + min(trunc(u * float(deg)), deg - 1)].
 * Step j >= 2.  Predecessor t = out[j-2], current v = out[j-1].  Up to max_attempts attempts of two words each: the first
 * word gives the candidate x = col[rs_v + o] as in step 1, the second gives r; accept if r < a, where a = a_ret if x == t,
 * else a_near if the value x occurs in row t of col (binary search over col[rs_t, re_t): the edge t -> x exists), else
 * a_far.  Row t is the rowptr pair validated when t was current; if t stayed (no valid row) the row is empty.  With
 * a_near == a_far the search is skipped.
 * Precondition.  col ascending within each row (duplicates and self loops allowed).  On unsorted rows the walk is still a
 * walk over edges and every read stays in bounds; only the bias is unspecified.
 * Fallback.  If all max_attempts attempts are rejected, one more word u draws exactly: position k of row v has the weight
 * a_ret / a_near / a_far of col[rs_v + k]; total = the sum of the weights in position order, in double;
 * target = double(u) * total; the first k whose double prefix sum exceeds target is taken, else deg - 1.  The running time
 * is therefore bounded for any p and q.  0 <= max_attempts <= 1024; 0 sends every biased step through the fallback.
 */
PYG_HIP_API int pyg_hip_node2vec_walk(int index_dtype, const void* rowptr, int64_t num_nodes, const void* col,
                                      int64_t num_edges, const void* seed, int64_t num_seeds, int64_t walk_length,
                                      float a_ret, float a_near, float a_far, uint64_t key, int max_attempts, void* out,
                                      void* stream);

/*
 * Edge lookup and negative sampling on a CSR graph (this build only; neither has an operator in the reference).  rowptr has
 * num_src + 1 entries, col num_edges; destinations are ids in [0, num_dst).  index_dtype is PYG_I32 or PYG_I64 and types
 * every buffer.  Both are pure functions of their arguments: the same on the device, on the binding's CPU key and in
 * tests/_negative_ref.py, bit for bit; integer arithmetic only.  One lane per item; no atomics, no allocation, no
 * synchronisation, no host read.
 *
 * Precondition.  col strictly ascending within each row (a coalesced graph).  On rows that break it every read stays in
 * bounds, every result is -1 or lies in the candidate range and all three implementations still agree (they run the same
 * loops); only "is not an edge" and uniformity are unspecified.  Every comparison below is meant in exact integers: the
 * device and the host code arrange theirs so that nothing overflows int64 whatever rowptr, col and ptr hold (kth clamps
 * W[mid] to [lo - 1, hi]; an empty range hi <= lo gives -1 before hi - lo is formed; the global bisection compares
 * rowptr[s + 1] with (s + 1) * num_dst - R).
 * A row is VALID if its source s lies in [0, num_src) and (rs, re) = (rowptr[s], rowptr[s+1]) has 0 <= rs <= re <= num_edges;
 * then row = col[rs, re).
 * lower_bound(W, x):  a = 0, b = |W|; while a < b: mid = (a + b) / 2; if W[mid] < x then a = mid + 1 else b = mid.  Result a.
 * kth(W, lo, r):      a = 0, b = |W|; while a < b: mid = (a + b) / 2; if W[mid] - lo - mid > r then b = mid else a = mid + 1.
 *                     Result lo + r + a: the r-th value of lo, lo + 1, ... that is not in W.
 *
 * pyg_hip_edge_lookup: out[q] = rs + lower_bound(row, dst[q]) if that position lies in the row and holds dst[q] -- the
 * first entry of row src[q] that equals dst[q] -- else -1; -1 also if row src[q] is not valid.
 *
 * pyg_hip_negative_sample.  Words: item t owns at::Philox4_32(key, subsequence = t, offset = 0), takes its first two words
 * and forms w = (w0 << 32) | w1; a draw below n is (w * n) >> 64, the high half of the 64 x 64 product (bias <= n / 2^64).
 *  src != NULL (structured): out is [num_items, num_neg], item t = i * num_neg + j.  out[i][j] is a destination x with
 *   (src[i], x) not an edge, x != src[i] if exclude_self, x in the graph of src[i] if ptr; -1 if there is none.
 *   1. s = src[i]; -1 unless row s is valid.
 *   2. [lo, hi) = [0, num_dst) without ptr.  With ptr (num_graphs + 1 entries): a = 0, b = num_graphs + 1; while a < b:
 *      mid = (a + b) / 2; if ptr[mid] <= s then a = mid + 1 else b = mid.  g = a - 1; -1 if g < 0 or g >= num_graphs;
 *      lo = max(ptr[g], 0), hi = min(ptr[g+1], num_dst).
 *   3. W = row[lower_bound(row, lo), lower_bound(row, hi)), d = |W| (0 if the bounds are reversed).
 *   4. self_ex = exclude_self && lo <= s < hi && s not in W (by lower_bound(W, s)).
 *   5. n = (hi - lo) - d - self_ex; -1 if n <= 0.  r = the draw below n; x = kth(W, lo, r); if self_ex && x >= s then
 *      x = kth(W, lo, r + 1).
 *  src == NULL (global), whatever num_items is -- a structured call without sources has no items and needs no call:
 *   num_items is ignored, out is [2, num_neg] (sources, then destinations), item t = j.  The pair is
 *   uniform over the non-edge cells of the num_src x num_dst matrix.  exclude_self and ptr must be 0 / NULL.
 *   1. T = num_src * num_dst - num_edges (must not overflow; sizes only); (-1, -1) if T <= 0.  R = the draw below T.
 *   2. s = the smallest row of [0, num_src) with (s + 1) * num_dst - rowptr[s + 1] > R: a = 0, b = num_src; while a < b:
 *      mid = (a + b) / 2; if (mid + 1) * num_dst - rowptr[mid + 1] > R then b = mid else a = mid + 1; s = a; (-1, -1) if
 *      s == num_src.
 *   3. r = R - (s * num_dst - rowptr[s]); (-1, -1) if row s is not valid or r lies outside [0, num_dst - (re - rs)).
 *   4. (s, kth(row, 0, r)).
 */
PYG_HIP_API int pyg_hip_edge_lookup(int index_dtype, const void* rowptr, int64_t num_src, const void* col, int64_t num_edges,
                                    const void* src, const void* dst, int64_t num_queries, void* out, void* stream);
PYG_HIP_API int pyg_hip_negative_sample(int index_dtype, const void* rowptr, int64_t num_src, const void* col,
                                        int64_t num_edges, const void* src, int64_t num_items, int64_t num_dst,
                                        int64_t num_neg, uint64_t key, int exclude_self, const void* ptr, int64_t num_graphs,
                                        void* out, void* stream);

/*
 * Induced subgraph of a node list.  Replaces pyg::subgraph (schema pyg_lib/csrc/sampler/subgraph.cpp:30-32; CPU kernel
 * sampler/cpu/subgraph_kernel.cpp:13-92 with the Mapper of sampler/cpu/mapper.h; the reference has no device kernel).
 * index_dtype is PYG_I32 or PYG_I64 and types rowptr (num_nodes + 1), col (num_edges), nodes (num_selected) and every
 * output.  out_rowptr (caller-allocated, num_selected + 1 entries) has one row per POSITION of `nodes`; the row holds
 * the kept neighbours of nodes[i] in CSR order.  The local id of a node is the rank of its first occurrence among the
 * distinct nodes of `nodes` (Mapper::insert order), so a duplicated node repeats its row and its id is that of the first
 * occurrence.  *out_col / *out_edge_id (positions in col of the kept edges; NULL unless return_edge_id) come from
 * host->alloc (only alloc / free of `host` are used) and hold *num_out_edges entries.  A node id outside
 * [0, num_nodes), in `nodes` or in col, is never a member (an entry of `nodes` gets an empty row and no local id).
 * Deterministic.  Synchronises `stream` once, to size the edge outputs (the reference reads out_rowptr[-1] the same
 * way); num_selected = 0 does not synchronise.
 */
PYG_HIP_API int pyg_hip_subgraph(int index_dtype, const void* rowptr, int64_t num_nodes, const void* col,
                                 int64_t num_edges, const void* nodes, int64_t num_selected, int return_edge_id,
                                 const pyg_hip_sampler_host* host, void* out_rowptr, void** out_col, void** out_edge_id,
                                 int64_t* num_out_edges, void* stream);

/* ---- index_sort ---------------------------------------------------------------------------- */

PYG_HIP_API size_t pyg_hip_index_sort_workspace_size(int dtype, int64_t n);

/*
 * Ascending STABLE sort of `n` integer keys: keys_out = sorted keys (same dtype), index_out =
 * int64 permutation, bit-identical to torch.sort(stable=True).
 * Replaces pyg::index_sort (schema pyg_lib/csrc/ops/index_sort.cpp:25-28; CPU kernel
 * pyg_lib/csrc/ops/cpu/index_sort_kernel.cpp:14-59 + ops/cpu/radix_sort.h:58-198; the reference
 * has no device kernel, pyg_lib/ops/__init__.py:319-320 falls back to torch.sort).
 *   dtype      PYG_U8 / PYG_I8 / PYG_I16 / PYG_I32 / PYG_I64 (anything else: "Input should contain
 *              integral values.", index_sort_kernel.cpp:55-56)
 *   max_value  with has_max != 0: an upper bound of the (non-negative) keys, only sets the number of
 *              8-bit passes (radix_sort.h:170-176).  With has_max == 0 the extremes are reduced on
 *              the device and read back (one stream synchronisation, like the reference's
 *              input.max().item()); negative keys are then sorted correctly as well.
 */
PYG_HIP_API int pyg_hip_index_sort(int dtype, const void* keys, int64_t n, int64_t max_value,
                                   int has_max, void* keys_out, int64_t* index_out, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---- scatter / segment_coo / gather_coo ---------------------------------------------------- */

typedef enum {
  PYG_REDUCE_SUM = 0,
  PYG_REDUCE_MUL = 1,
  PYG_REDUCE_MIN = 2,
  PYG_REDUCE_MAX = 3
} pyg_reduce;

/*
 * out[b, index(b, e, k), k]  (op)=  src[b, e, k]      over the (B, E, K) view of `src`
 * (layout of pyg_lib/csrc/ops/cpu/scatter_kernel.cpp:16-24; `out` is [B, N, K]).
 * Replaces pyg::scatter_{sum,mul,min,max} (schemas pyg_lib/csrc/ops/scatter.cpp:156-172; CPU
 * kernels ops/cpu/scatter_kernel.cpp:29-511; CUDA ops/cuda/scatter_kernel.cu:56-651) and, with a
 * sorted [B, E] index, pyg::segment_{sum,min,max}_coo (schemas ops/segment_coo.cpp:150-165; CPU
 * ops/cpu/segment_coo_kernel.cpp:31-651; CUDA ops/cuda/segment_coo_kernel.cu:73-1301).
 *   index     int64, element (b, e, k) at index[b*stride_b + e*stride_e + k*stride_k]; a stride of
 *             0 broadcasts (1-D index: (0, 1, 0); COO index [B, E]: (E, 1, 0); fully expanded:
 *             (E*K, K, 1)).
 *   out       running state, updated in place (`out=` contract, ops/scatter.h:11-113): the caller
 *             pre-fills it (zeros / ones / pyg_hip_fill_reduce_identity for fresh outputs).
 *   MIN/MAX   arg_out [B, N, K] int64 is filled here: source position of the first element that
 *             produced the final value, or the sentinel E.  out_init = NULL means `out` was filled
 *             with the reduce identity: empty buckets are then reset to 0
 *             (scatter_kernel.cpp:351-360).  Otherwise out_init points to a copy of the caller's
 *             initial `out` and untouched buckets keep their value.
 *   index_sorted  flag bits:
 *             bit 0 (PYG_HIP_SCATTER_SORTED) promises an ascending index along e (the COO contract).
 *             Bit 1 (PYG_HIP_SCATTER_FRESH_SUM, SUM only): `out` is a fresh, UNINITIALISED output -- the rows routes
 *             write every slot without reading or clearing it (2 x N x K bytes less traffic), the other routes clear it.
 *             Bit 2 (PYG_HIP_SCATTER_CAS): the atomic sums add floats / doubles / packed 16-bit pairs through
 *             compare-and-swap loops instead of the hardware's floating-point atomic adds (a flavour, not a route).
 *             Bit 3 (PYG_HIP_SCATTER_DETERMINISTIC): no floating-point atomics -- see the table.  Ignored for integer
 *             types and for MIN / MAX (exact on every route).  The torch binding sets it when
 *             torch.are_deterministic_algorithms_enabled().
 *   workspace optional scratch of pyg_hip_scatter_workspace_size(B, E, N) bytes for the rows routes; NULL, or fewer
 *             bytes than the route needs (csr_rows: the B x (N + 1) row offsets, a multiple of 256 bytes; sort_rows:
 *             the full size for B = 1), means "not offered" and the call takes the route it would take without one.
 *
 * The route of a call -- the first line that applies (pyg_hip_scatter_route asks, pyg_hip_scatter_last_route tells):
 *   none          B x E x K == 0
 *   csr_rows      SUM / MIN / MAX, index broadcast along k (stride_k == 0), SORTED, workspace: buckets are CSR rows
 *   sort_rows     SUM / MIN / MAX, stride_k == 0, not SORTED, ONE index vector (B == 1, stride_e == 1), workspace, and
 *                   MIN / MAX:            E >= 2^15
 *                   SUM f32 / f16 / bf16: E >= 2^15 and rows of >= 64 bytes
 *                   SUM, DETERMINISTIC:   any E, row width and floating type (float64 included)
 *                 -- one stable index sort, CSR rows read through the permutation
 *   unsupported   DETERMINISTIC, floating SUM or MUL: pyg_hip_scatter returns PYG_HIP_ERR_UNSUPPORTED (element-wise
 *                 indices, B > 1 unsorted, no workspace; floating MUL always)
 *   atomic        MIN / MAX: integer atomics / a CAS loop on the reference's `<` / `>`, an arg pass, reset of empty buckets
 *   elem          MUL: CAS loop per element
 *   vec_sorted / vec_unsorted   SUM f32 / f16 / bf16, stride_k == 0, rows of whole 16-byte slices, src and out 16-byte
 *                 aligned, and SORTED or more than four slices per row: a thread owns a slice over 32 / 8 positions
 *   pair          SUM f16 / bf16, stride_k == 0, K even, not SORTED, src and out 4-byte aligned: one packed add per pair
 *   elem          every other SUM (float64, integers, element-wise indices, ...): one native atomic (8- / 16-bit: a CAS
 *                 loop) per element
 * The rows routes reduce every bucket in SOURCE order without atomics: deterministic, the same bits in every run like the
 * reference's sequential CPU loop (ops/cpu/scatter_kernel.cpp:29-127), fp32 accumulation with one rounding per output,
 * every output row written once; min / max: no CAS loops, no second arg pass, same exact values and first-match arg.
 * Non-finite values and signed zeros follow the reference's sequential loops on every path: a NaN never
 * wins a min / max (a bucket of NaN only counts as empty) and makes a sum NaN; +0 and -0 tie, the first one seen stays
 * (value bits and arg, also on the atomic path); a sum of nothing but -0 into a caller's -0 stays -0, into a fresh output
 * it is +0; denormal sums are kept.
 */
#define PYG_HIP_SCATTER_SORTED 1
#define PYG_HIP_SCATTER_FRESH_SUM 2
#define PYG_HIP_SCATTER_CAS 4
#define PYG_HIP_SCATTER_DETERMINISTIC 8
#define PYG_HIP_SCATTER_ROUTE_NONE 0
#define PYG_HIP_SCATTER_ROUTE_CSR_ROWS 1
#define PYG_HIP_SCATTER_ROUTE_SORT_ROWS 2
#define PYG_HIP_SCATTER_ROUTE_VEC_SORTED 3
#define PYG_HIP_SCATTER_ROUTE_VEC_UNSORTED 4
#define PYG_HIP_SCATTER_ROUTE_PAIR 5
#define PYG_HIP_SCATTER_ROUTE_ELEM 6
#define PYG_HIP_SCATTER_ROUTE_ATOMIC 7
#define PYG_HIP_SCATTER_ROUTE_UNSUPPORTED 8
PYG_HIP_API size_t pyg_hip_scatter_workspace_size(int64_t B, int64_t E, int64_t N);
/* The table above as a query: the PYG_HIP_SCATTER_ROUTE_* code pyg_hip_scatter would take for these scalar arguments, a
 * workspace of `workspace_bytes` bytes (0: none) and `misalign` = the low four bits of (src | out), which only decide among
 * vec_*, pair and elem.  An unknown op or dtype or a negative size answers PYG_HIP_SCATTER_ROUTE_UNSUPPORTED.  Launches
 * nothing and needs no device: like pyg_hip_scatter_workspace_size it reads the current device's compute-unit count (the
 * sort's scratch depends on it) and assumes an MI355X where there is none. */
PYG_HIP_API int pyg_hip_scatter_route(int op, int dtype, int64_t index_stride_b, int64_t index_stride_e,
                                      int64_t index_stride_k, int64_t B, int64_t E, int64_t K, int64_t N,
                                      int flags, size_t workspace_bytes, unsigned misalign);
/* Name of the route ("csr_rows", ... as in the table; "none" for a call that did nothing or failed its argument checks)
 * the last pyg_hip_scatter call on this thread took: lets tests assert which kernel ran. */
PYG_HIP_API const char* pyg_hip_scatter_last_route(void);
PYG_HIP_API int pyg_hip_scatter(int op, int dtype, const void* src, const int64_t* index,
                                int64_t index_stride_b, int64_t index_stride_e,
                                int64_t index_stride_k, void* out, int64_t* arg_out,
                                const void* out_init, int64_t B, int64_t E, int64_t K, int64_t N,
                                int index_sorted, void* workspace, size_t workspace_bytes,
                                void* stream);

/* Fill `n` elements with numeric_limits<T>::max() (MIN) / lowest() (MAX): the start state of a
 * fresh min/max output (scatter_kernel.cpp:296-300). */
PYG_HIP_API int pyg_hip_fill_reduce_identity(int op, int dtype, void* out, int64_t n, void* stream);

/*
 * out[b, e, k] = src[b, index[b, e], k]     src [B, N, K], index [B, E] contiguous, out [B, E, K].
 * Replaces pyg::gather_coo (schema ops/segment_coo.cpp:164-165; CPU
 * ops/cpu/segment_coo_kernel.cpp:666-746; CUDA ops/cuda/segment_coo_kernel.cu:1316-1444).
 */
PYG_HIP_API int pyg_hip_gather_coo(int dtype, const void* src, const int64_t* index, void* out,
                                   int64_t B, int64_t E, int64_t K, int64_t N, void* stream);

/* ---- sampled_op ----------------------------------------------------------------------------- */

typedef enum {
  PYG_SAMPLED_ADD = 0,
  PYG_SAMPLED_SUB = 1,
  PYG_SAMPLED_MUL = 2,
  PYG_SAMPLED_DIV = 3
} pyg_sampled_fn;

/*
 * out[e, :] = left[li(e), :]  (fn)  right[ri(e), :]     for e in [0, E);  li(e) = left_index ? left_index[e] : e, ri alike.
 * Replaces pyg::sampled_op (schema pyg_lib/csrc/ops/sampled.cpp:57-59; CPU kernel ops/cpu/sampled_kernel.cpp:17-46 =
 * index_select + operator; CUDA kernel ops/cuda/sampled_kernel.cu:21-106, int64 indices only): the gathered operands
 * left[left_index] and right[right_index] never exist in memory.
 *   left [left_rows, F], right [right_rows, F], out [E, F], row-major, all `dtype`.
 *   index_dtype  PYG_I64 or PYG_I32, the type of BOTH index vectors (E entries each; NULL = the identity, then the table
 *                has at least E rows).
 *   Floating dtypes take all four operators; bf16 / fp16 compute in fp32 and round once to nearest-even (torch's CPU
 *   kernels: same bits, Inf / NaN / signed zeros / denormals included; the division is the correctly rounded one).
 *   Integer dtypes take add / sub / mul with wrap-around; PYG_SAMPLED_DIV on them returns PYG_HIP_ERR_UNSUPPORTED without a
 *   launch (the reference's backends disagree there -- true division on the CPU, truncation in CUDA -- and a zero divisor
 *   must not reach the device).
 *   Indices are NOT validated on the device (as pyg_hip_gather_coo and the reference's CUDA kernel): an index outside
 *   [0, left_rows) / [0, right_rows) is an out-of-bounds read; left_rows / right_rows only serve the identity check above.
 *   E == 0 or F == 0: PYG_HIP_OK without a launch.  Never synchronises.
 */
PYG_HIP_API int pyg_hip_sampled_op(int fn, int dtype, const void* left, int64_t left_rows, const void* right,
                                   int64_t right_rows, int index_dtype, const void* left_index, const void* right_index,
                                   void* out, int64_t E, int64_t F, void* stream);

/*
 * Per-edge gradients of pyg_hip_sampled_op for PYG_SAMPLED_MUL / PYG_SAMPLED_DIV, floating dtypes only (add / sub need none:
 * their edge gradient is grad_out itself).  With g = grad_out[e], a = left[li(e)], b = right[ri(e)] -- each read once --
 *   mul:  edge_grad_left = g * b      edge_grad_right = g * a
 *   div:  edge_grad_left = g / b      edge_grad_right = (-g) * ((a / b) / b)
 * in that operation order (SampledOp::backward, pyg_lib/csrc/ops/autograd/sampled_kernel.cpp:55-82), in opmath (fp32 for
 * the 16-bit types) with ONE rounding on store -- the reference rounds every intermediate to `dtype`.  Either output may
 * be NULL (not wanted); both are [E, F].  The sum over the edges of a node (the reference's index_select_backward) is
 * the caller's: pyg_hip_scatter.  Indices are not validated, as above.
 */
PYG_HIP_API int pyg_hip_sampled_op_backward(int fn, int dtype, const void* grad_out, const void* left, int64_t left_rows,
                                            const void* right, int64_t right_rows, int index_dtype,
                                            const void* left_index, const void* right_index, void* edge_grad_left,
                                            void* edge_grad_right, int64_t E, int64_t F, void* stream);

/* ---- fused_scatter_reduce ------------------------------------------------------------------- */

typedef enum {
  PYG_FUSED_SUM = 0,
  PYG_FUSED_MEAN = 1,
  PYG_FUSED_MIN = 2,
  PYG_FUSED_MAX = 3
} pyg_fused_reduce;

/*
 * out[n, k * F + f] = reduce_{ops[k]} over { src[e, f] : index[e] == n }      for k in [0, n_ops), n in [0, N)
 * Replaces pyg_lib.ops.scatter_reduce.fused_scatter_reduce (pyg_lib/ops/scatter_reduce.py:95-181, a Triton kernel: float
 * atomics, no backward) and four separate pyg_hip_scatter calls on the same index: ONE stable index sort, ONE pass over the
 * rows with a sum, a min and a max accumulator per element, the count from the row offsets.  No float atomics: the same bits
 * on every run.
 *   src [E, F] row-major, floating `dtype` only (PYG_F32 / F64 / F16 / BF16; others: PYG_HIP_ERR_UNSUPPORTED);
 *   index [E] int64; out [N, n_ops * F] row-major, every element written (need not be cleared).
 *   ops       n_ops = 1 ... 4 distinct codes of pyg_fused_reduce in any order; slice k of an output row holds ops[k].  An
 *             empty list, an unknown code or a duplicate: PYG_HIP_ERR_INVALID, nothing launched.
 *   arg_min / arg_max  NULL (not wanted: no position is tracked) or int64 [N, F]: source position of the first element that
 *             produced the value, or the sentinel E.  Ignored when the reduction is not listed.
 *   count_out NULL or int64 [N]: entries per bucket.
 *   workspace pyg_hip_fused_scatter_reduce_workspace_size(dtype, E, N, F) bytes, 8-byte aligned; less is PYG_HIP_ERR_INVALID
 *             (there is no second path).
 * A bucket is reduced in SOURCE order in opmath (fp32 for the 16-bit types and float32, fp64 for float64) with one rounding
 * on store; mean = (opmath sum) / max(count, 1), rounded once.  Buckets split over lanes or hub chunks combine by a fixed
 * tree (sums then differ from the sequential order by rounding only; min / max and their positions never).  Empty buckets
 * read 0 in every slice.  Non-finite values and signed zeros as pyg_hip_scatter above (fresh output): strict
 * compares, a NaN never wins a min / max, a bucket of NaN only (or one that never beats the start value, the type's largest /
 * lowest finite number) reads 0 with the sentinel; +0 and -0 tie and the first position wins; a NaN, or +Inf with -Inf,
 * makes sum and mean NaN; a sum of nothing but -0 reads +0.
 * `index` is NOT validated on the device.  The forward uses it as a sort key only -- an entry outside [0, N) is never turned
 * into an address, but it is sorted by its low bits and the results of any bucket may then be wrong.
 * E == 0, F == 0 or N == 0: PYG_HIP_OK, a non-empty output is cleared, `src` and `index` are not touched.  Never synchronises
 * (N bounds the sort keys: no read-back); capturable in a HIP graph.
 */
PYG_HIP_API size_t pyg_hip_fused_scatter_reduce_workspace_size(int dtype, int64_t E, int64_t N, int64_t F);
PYG_HIP_API int pyg_hip_fused_scatter_reduce(int dtype, const void* src, const int64_t* index, int64_t E, int64_t F, int64_t N,
                                             const int* ops, int n_ops, void* out, int64_t* arg_min, int64_t* arg_max,
                                             int64_t* count_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Backward of pyg_hip_fused_scatter_reduce (the reference has none), one pass over the edges, no atomics, every element of
 * grad_in [E, F] written once:
 *   grad_in[e, f] = sum over k in list order of
 *     sum :  g_k[index[e], f]
 *     mean:  g_k[index[e], f] / max(count[index[e]], 1)
 *     min :  arg_min[index[e], f] == e ? g_k[index[e], f] : 0          max: likewise with arg_max
 * g_k = columns [k * F, (k + 1) * F) of grad_out [N, n_ops * F]; accumulated from +0 in opmath, one rounding.  The whole
 * gradient of a min / max goes to the first-match position, as in pyg::scatter_min / scatter_max.  arg_min / arg_max / count
 * are what the forward wrote and are required for the reductions listed (else PYG_HIP_ERR_INVALID).  Here index[e] IS an
 * address: an entry outside [0, N) is an out-of-bounds read.  E == 0 or F == 0: PYG_HIP_OK without a launch.  Never
 * synchronises.
 */
PYG_HIP_API int pyg_hip_fused_scatter_reduce_backward(int dtype, const void* grad_out, const int64_t* index,
                                                      const int64_t* arg_min, const int64_t* arg_max, const int64_t* count,
                                                      int64_t E, int64_t F, int64_t N, const int* ops, int n_ops, void* grad_in,
                                                      void* stream);

/* ---- knn, radius, nearest: batched point-cloud neighbour search -------------------------------------------------
 *
 * Replace pyg::knn / pyg::radius / pyg::nearest (schemas ops/{knn,radius,nearest}.cpp; CUDA ops/cuda/{knn,radius,nearest}_kernel.cu).
 * knn and radius: x [N, D] are the candidates, y [M, D] the queries; nearest: x [N, D] are the queries, y [M, D] the candidates.
 * Row-major, one floating `dtype` (PYG_F32 / F64 / F16 / BF16) for both, 1 <= D <= 4096.  ptr_x / ptr_y: int64 CSR pointers of
 * num_examples + 1 entries on the device; NULL means the single example [0, rows] (num_examples must then be 1 for both).
 * Example b pairs the queries ptr_q[b] .. ptr_q[b + 1] with the candidates ptr_c[b] .. ptr_c[b + 1].
 *
 * Distance: squared Euclidean, dist = 0; for d = 0 .. D-1: diff = a[d] - b[d]; dist = dist + diff * diff -- every operation
 * rounded on its own, NO fused multiply-add, in fp32 (fp64 for PYG_F64; 16-bit inputs are widened exactly).  This is the
 * arithmetic of the reference's CPU `nearest` loop, so the device and a plain CPU loop agree bit for bit, near-ties included.
 * A candidate at distance NaN or +Inf is never returned by any of the three.
 *
 * knn:     per query i (ascending) the eligible candidates of its example ordered by (distance, index); the first
 *          min(k, eligible) become columns (i, j) of out [2, E].  1 <= k <= 100 (more: PYG_HIP_ERR_UNSUPPORTED, the
 *          reference's limit).  PYG_HIP_SPATIAL_COSINE: the distance is 1 - dot / (|x| |y|), norms computed once per point.
 * radius:  a candidate matches when dist < (compute type)(r * r), the product formed in double; per query the first
 *          max_num_neighbors matches in ascending candidate index are kept; PYG_HIP_SPATIAL_IGNORE_SAME drops j == i (global
 *          indices); out [2, E] ordered by (i, j) -- the rule of the reference's CUDA kernel.
 * nearest: out[i] = the first index of the example's y range at the smallest eligible distance; a query without an eligible
 *          candidate gets the clamped ptr_y[b] (which can equal M).
 *
 * Pointers: every segment bound is clamped into [0, rows] before use, so a bad pointer never causes an access outside the
 * buffers.  A pointer that decreases, or whose last entry is not the row count, is reported: by knn / radius in the call
 * (PYG_HIP_ERR_INVALID; they read the pair count back anyway), by nearest -- which never synchronises -- through a pinned
 * word of the device: the NEXT pyg_hip_nearest call on that device fails with PYG_HIP_ERR_INVALID, and
 * pyg_hip_nearest_pending_error() returns and clears the word (meaningful once the stream has been synchronised).
 *
 * Two calls for knn and radius, because the caller allocates the output: pyg_hip_knn / pyg_hip_radius run the search into the
 * workspace, wait for `stream` once and return the pair count E in *num_pairs (host); pyg_hip_knn_emit / pyg_hip_radius_emit,
 * given the SAME arguments and workspace, write out [2, E] (int64) without synchronising.  Everything is queued on `stream`.
 * Fewer than 2^31 rows in x and in y (PYG_HIP_ERR_UNSUPPORTED otherwise: indices inside the kernels are 32-bit); pair counts
 * and output offsets are 64-bit.  workspace: pyg_hip_spatial_workspace_size(...) bytes for the same arguments and flags,
 * 16-byte aligned; less is PYG_HIP_ERR_WORKSPACE.
 *
 * Routes.  pyg_hip_spatial_route(op, dtype, M, N, B, D, k) -- M queries, N candidates, B examples -- answers, without touching
 * a device, which route a call without a FORCE flag takes; pyg_hip_spatial_last_route() names what the last call on this
 * thread ran: "<op> <lane|split> <d4|ldsq|globq> <reg1|reg16|lds|count>[ cosine]".
 *   lane   one workgroup per tile of 128 queries scans the example's whole candidate range through LDS.
 *   split  fewer than 256 query tiles (M < 32768: under one workgroup per CU) AND at least 512 candidates per example on
 *          average: the candidate range is cut into up to 64 chunks, a (tile, chunk) grid leaves sorted partial lists (counts
 *          for radius) and a second launch merges them by (distance, index).  No atomics: repeated calls give the same bits.
 * The rule is monotone in M.  PYG_HIP_SPATIAL_FORCE_LANE / _FORCE_SPLIT override it (tests, measurements); forced, the
 * split route's shortest chunk is 32 candidates instead of 256, so that small inputs span several chunks.
 * pyg_hip_spatial_tile(which) returns the kernels' tile constants (PYG_HIP_SPATIAL_TILE_*), for tests that probe their edges.
 */
#define PYG_SPATIAL_KNN 0
#define PYG_SPATIAL_RADIUS 1
#define PYG_SPATIAL_NEAREST 2
#define PYG_HIP_SPATIAL_FORCE_LANE 1
#define PYG_HIP_SPATIAL_FORCE_SPLIT 2
#define PYG_HIP_SPATIAL_COSINE 4
#define PYG_HIP_SPATIAL_IGNORE_SAME 8
#define PYG_HIP_SPATIAL_ROUTE_UNSUPPORTED 0
#define PYG_HIP_SPATIAL_ROUTE_LANE 1
#define PYG_HIP_SPATIAL_ROUTE_SPLIT 2
#define PYG_HIP_SPATIAL_TILE_QUERIES 0      /* queries per workgroup */
#define PYG_HIP_SPATIAL_TILE_CANDIDATES 1   /* candidates per LDS tile, D <= 4 */
#define PYG_HIP_SPATIAL_TILE_CHUNK_FORCED 2 /* shortest chunk of a forced split */
#define PYG_HIP_SPATIAL_TILE_ELEMS 3        /* elements per LDS tile, D > 4 (rows = max(1, elems / D)) */
PYG_HIP_API int pyg_hip_spatial_route(int op, int dtype, int64_t M, int64_t N, int64_t B, int64_t D, int64_t k);
PYG_HIP_API const char* pyg_hip_spatial_last_route(void);
PYG_HIP_API int pyg_hip_spatial_tile(int which);
PYG_HIP_API size_t pyg_hip_spatial_workspace_size(int op, int dtype, int64_t M, int64_t N, int64_t B, int64_t D, int64_t k,
                                                  int flags);
PYG_HIP_API int pyg_hip_knn(int dtype, const void* x, int64_t N, const void* y, int64_t M, int64_t D, const int64_t* ptr_x,
                            const int64_t* ptr_y, int64_t num_examples, int64_t k, int flags, void* workspace,
                            size_t workspace_bytes, int64_t* num_pairs, void* stream);
PYG_HIP_API int pyg_hip_knn_emit(int dtype, int64_t N, int64_t M, int64_t D, int64_t num_examples, int64_t k, int flags,
                                 const void* workspace, size_t workspace_bytes, int64_t num_pairs, int64_t* out, void* stream);
PYG_HIP_API int pyg_hip_radius(int dtype, const void* x, int64_t N, const void* y, int64_t M, int64_t D, const int64_t* ptr_x,
                               const int64_t* ptr_y, int64_t num_examples, double r, int64_t max_num_neighbors, int flags,
                               void* workspace, size_t workspace_bytes, int64_t* num_pairs, void* stream);
PYG_HIP_API int pyg_hip_radius_emit(int dtype, const void* x, int64_t N, const void* y, int64_t M, int64_t D, const int64_t* ptr_x,
                                    const int64_t* ptr_y, int64_t num_examples, double r, int64_t max_num_neighbors, int flags,
                                    void* workspace, size_t workspace_bytes, int64_t num_pairs, int64_t* out, void* stream);
PYG_HIP_API int pyg_hip_nearest(int dtype, const void* x, int64_t N, const void* y, int64_t M, int64_t D, const int64_t* ptr_x,
                                const int64_t* ptr_y, int64_t num_examples, int flags, void* workspace, size_t workspace_bytes,
                                int64_t* out, void* stream);
PYG_HIP_API int pyg_hip_nearest_pending_error(void);

/* ---- fps, grid_cluster: point-cloud downsampling -------------------------------------------------------------------
 *
 * Replace pyg::fps and pyg::grid_cluster (schemas ops/fps.cpp, ops/cluster.cpp; CUDA ops/cuda/{fps,cluster}_kernel.cu).
 *
 * fps -- farthest point sampling.  src [N, D] row-major, one floating `dtype` (PYG_F32 / F64 / F16 / BF16), 1 <= D <= 4096;
 * ptr: int64 [B + 1] on the device, example b owns the points ptr[b] .. ptr[b + 1]; out_ptr: int64 [B] on the device, the
 * running sum of the per-example sample counts (the reference's cumsum: example b writes out[out_ptr[b - 1] .. out_ptr[b]),
 * out_ptr[-1] read as 0); start: int64 [B] on the device, the local index of every example's first sample, clamped into its
 * example (NULL: zeros).  out: int64 [out_total], global point indices, example after example.
 *   distance   squared Euclidean, dist = 0; for d = 0 .. D-1: diff = a[d] - b[d]; dist = dist + diff * diff -- every operation
 *              rounded on its own, NO fused multiply-add, in fp32 (fp64 for PYG_F64; 16-bit inputs are widened exactly): the
 *              arithmetic of knn / radius / nearest.
 *   running    run[i] = dist(i, first sample); after every further sample s: new = dist(i, s); run[i] = new < run[i] ? new : run[i].
 *              A point whose first distance is NaN keeps a NaN.
 *   next       the point with the largest run[i]; among equals the lowest index; a NaN ranks below every number.  Once all
 *              running distances are 0 (duplicates, an exhausted example) the example's lowest index repeats, as an argmax over
 *              zeros does.
 * An example without points writes nothing.  No atomics: every route, every call and the CPU key give the same bits.
 * N < 2^31 (PYG_HIP_ERR_UNSUPPORTED otherwise, and for D > 4096).
 *
 * The caller promises max_points >= the largest example and max_samples >= the largest count (they size the launch; the
 * binding computes both on the device and reads them back in one copy).  Nothing outside a buffer is ever touched: pointer
 * entries are clamped into [0, N], write offsets into [0, out_total], an example longer than max_points is cut to it, and no
 * example writes more than max_samples indices.  Any of these, a ptr that decreases, does not begin at 0 or does not end at N,
 * sets a pinned word of the device -- fps never synchronises --: the NEXT pyg_hip_fps call on that device fails with
 * PYG_HIP_ERR_INVALID, and pyg_hip_fps_pending_error() returns and clears the word (meaningful once the stream has been
 * synchronised).
 *
 * Routes.  pyg_hip_fps_route(dtype, B, D, max_points, max_samples, flags) answers, without touching a device, which route a
 * call takes (PYG_HIP_FPS_ROUTE_*); pyg_hip_fps_last_route() names what the last call on this thread ran:
 * "resident <d4|lds|glob> t<threads>", "stream <d4|glob>" or "multi <d4|glob> g<blocks per example>".
 *   resident   one workgroup per example, 64 .. 1024 threads picked from max_points; a thread keeps the running distances of its
 *              PYG_HIP_FPS_TILE_POINTS points in registers for the whole call and an iteration costs ONE barrier.  d4 (D <= 4):
 *              the coordinates live in registers too and the winner's travel with its key; lds / glob (any D): they are
 *              re-read every iteration from an LDS copy of the example while it fits PYG_HIP_FPS_TILE_LDS_BYTES, else from
 *              global memory.
 *   stream     max_points above the resident capacity (1024 * PYG_HIP_FPS_TILE_POINTS): the same loop with 1024 threads, the
 *              running distances in the workspace.
 *   multi      fewer than PYG_HIP_FPS_TILE_MULTI_EXAMPLES examples AND max_points >= PYG_HIP_FPS_TILE_MULTI_POINTS: one plain
 *              launch per sample with grid (G, B); every block first reduces the G partial keys of the previous launch
 *              (redundantly: no second launch, no spin, no grid barrier), block 0 writes the sample, then the block updates
 *              its slice of the running distances and leaves its partial key for the next launch.  max_samples launches, no
 *              synchronisation.
 * PYG_HIP_FPS_FORCE_RESIDENT / _STREAM / _MULTI override the rule (tests, measurements): a forced resident call whose
 * max_points exceeds the capacity takes `stream`; a forced multi call cuts slices as short as PYG_HIP_FPS_TILE_SLICE_FORCED
 * points so that small inputs span several blocks.  pyg_hip_fps_tile(which) returns the constants (PYG_HIP_FPS_TILE_*).
 * workspace: pyg_hip_fps_workspace_size(...) bytes for the same arguments and flags, 16-byte aligned.
 *
 * grid_cluster -- voxel ids.  pos [N, D] row-major in `dtype` (the same four), size / start / end [D] in the same dtype on the
 * device; start == NULL: the column minimum of pos, end == NULL: the column maximum (a NaN in a column makes its bound NaN, as
 * torch.min / torch.max).  With R = rounding to `dtype` (the identity for F32 / F64, whose arithmetic is fp32 / fp64; the
 * 16-bit types compute in fp32 and round after each operation):
 *   q_d = int64(trunc(R(R(pos_d - start_d) / size_d))),  n_d = int64(trunc(R(R(end_d - start_d) / size_d))) + 1,
 *   out[i] = sum_d q_d * prod_{e < d} n_e   in wrapping int64 -- the reference's CUDA kernel, and its CPU kernel for D >= 2.
 * int64() of a NaN is 0 and saturates outside the int64 range (on the CPU key too); such ids mean nothing, and no address
 * depends on them.  One launch when both bounds are given; otherwise a first launch leaves per-block column minima / maxima in
 * the workspace and the second one reduces them in its prologue (every block, redundantly; no atomics).  Never synchronises.
 * workspace: pyg_hip_grid_cluster_workspace_size(dtype, N, D, have_start, have_end) bytes (0 when both bounds are given).
 */
#define PYG_HIP_FPS_FORCE_RESIDENT 1
#define PYG_HIP_FPS_FORCE_STREAM 2
#define PYG_HIP_FPS_FORCE_MULTI 3
#define PYG_HIP_FPS_FORCE_MASK 3
#define PYG_HIP_FPS_ROUTE_UNSUPPORTED 0
#define PYG_HIP_FPS_ROUTE_RESIDENT 1
#define PYG_HIP_FPS_ROUTE_STREAM 2
#define PYG_HIP_FPS_ROUTE_MULTI 3
#define PYG_HIP_FPS_TILE_POINTS 0         /* points per thread of the resident route */
#define PYG_HIP_FPS_TILE_MIN_THREADS 1    /* smallest resident workgroup */
#define PYG_HIP_FPS_TILE_MAX_THREADS 2    /* largest resident workgroup; the stream route's */
#define PYG_HIP_FPS_TILE_SLICE_FORCED 3   /* shortest slice of a forced multi call */
#define PYG_HIP_FPS_TILE_LDS_BYTES 4      /* resident, D > 4: the example's points are copied to LDS up to this size */
#define PYG_HIP_FPS_TILE_MULTI_POINTS 5   /* multi: max_points from here on ... */
#define PYG_HIP_FPS_TILE_MULTI_EXAMPLES 6 /* ... and fewer examples than this */
#define PYG_HIP_FPS_TILE_SLICE 7          /* shortest slice the rule cuts */
PYG_HIP_API int pyg_hip_fps_route(int dtype, int64_t B, int64_t D, int64_t max_points, int64_t max_samples, int flags);
PYG_HIP_API const char* pyg_hip_fps_last_route(void);
PYG_HIP_API int pyg_hip_fps_tile(int which);
PYG_HIP_API size_t pyg_hip_fps_workspace_size(int dtype, int64_t N, int64_t B, int64_t D, int64_t max_points, int64_t max_samples,
                                              int flags);
PYG_HIP_API int pyg_hip_fps(int dtype, const void* src, int64_t N, int64_t D, const int64_t* ptr, int64_t B, const int64_t* out_ptr,
                            const int64_t* start, int64_t max_points, int64_t max_samples, int flags, void* workspace,
                            size_t workspace_bytes, int64_t* out, int64_t out_total, void* stream);
PYG_HIP_API int pyg_hip_fps_pending_error(void);
PYG_HIP_API size_t pyg_hip_grid_cluster_workspace_size(int dtype, int64_t N, int64_t D, int have_start, int have_end);
PYG_HIP_API int pyg_hip_grid_cluster(int dtype, const void* pos, int64_t N, int64_t D, const void* size, const void* start,
                                     const void* end, void* workspace, size_t workspace_bytes, int64_t* out, void* stream);

/* ---- spline_basis, spline_weighting: the operators behind SplineConv ------------------------------------------------
 *
 * Replace the six pyg::spline_* operators (schemas ops/spline.cpp; CPU ops/cpu/spline_kernel.cpp; CUDA ops/cuda/spline_kernel.cu).
 * All tensors row-major and contiguous.  weight_index and kernel_size are int64, is_open_spline is uint8, all on the device.
 *
 * basis -- pseudo [E, D] in PYG_F32 / PYG_F64 (others: PYG_HIP_ERR_INVALID), degree 1, 2 or 3, D <= 16, S = (degree + 1)^D;
 * outputs basis [E, S] and weight_index [E, S].  For pair (e, s), with k = s, wi = 0, offset = 1, b = 1, for d = 0 .. D-1:
 *   k_mod = k % (degree + 1), k /= degree + 1
 *   v  = pseudo[e, d] * T(kernel_size[d] - degree * is_open_spline[d])          (the integer converted to the dtype)
 *   wi += ((int64(v) + k_mod) % kernel_size[d]) * offset, offset *= kernel_size[d]   (C truncation and C remainder: a pseudo
 *        outside [0, 1] can give a negative index, as in the reference; kernel_size[d] == 0 contributes 0)
 *   v -= floor(v);  b *= B(v, k_mod)
 * B is the uniform B-spline piece of the degree and B' (basis_backward) its derivative, written with the reference's double
 * literals, so that the promotion rules decide what is evaluated in double and rounded once exactly as there; no fused
 * multiply-add.  basis_backward: grad_pseudo[e, d] = (sum over s, in order, of B'(v_d) * prod_{d' != d} B(v_d') * grad_basis[e, s])
 * * T(kernel_size[d] - degree * is_open_spline[d]), the product running over d' in ascending order.  One launch each, one
 * thread per (e, s) / (e, d), no synchronisation.  The CPU key computes the same bits.
 *
 * weighting -- x [E, M_in], weight [K, M_in, M_out], basis / weight_index [E, S], PYG_F32 / PYG_F64 / PYG_BF16.  Every sum is
 * sequential from +0 in the order written, every product rounded on its own (no fused multiply-add), no atomics:
 *   forward          out[e, o]  = sum_s sum_i  w[wi, i, o] * (b[e, s] * x[e, i])
 *   backward_x       gx[e, i]   = sum_o sum_s  (g[e, o] * b[e, s]) * w[wi, i, o]
 *   backward_basis   gb[e, s]   = sum_o  g[e, o] * (sum_i w[wi, i, o] * x[e, i])
 *   backward_weight  gw[k, i, o] = sum over the pairs (e, s) with wi == k, in order of e then s, of (g[e, o] * b[e, s]) * x[e, i]
 * PYG_F32 / PYG_F64: the bits of the CPU key (backward_weight: for every weight of at most PYG_HIP_SPLINE_TILE_CHUNK pairs; a
 * longer one is summed chunk by chunk and the chunk sums are added in chunk order -- the same bits on every device and every
 * call, within gamma_(n+2) * sum|terms| of the exact sum).  PYG_BF16: the sums are kept in fp32 (the products of bfloat16
 * inputs are exact there) and rounded once at the end; the CPU key rounds every step to bfloat16 as the reference does.
 *
 * forward, backward_x and backward_basis are one kernel template: a 256-thread workgroup owns a tile of edges, lanes run along
 * the contiguous axis of the weights (backward_x first writes the transposed weights into its workspace), the tile's rows,
 * basis and weight_index go through LDS.  Two routes, pyg_hip_spline_route(dtype, E, S, M_in, M_out, K) -- pure, no device:
 *   global   the rule's answer for every supported shape: one workgroup per tile, the weights come through L2;
 *   lds      only when forced (PYG_HIP_SPLINE_FORCE_LDS) and K * M_in * M_out elements fit PYG_HIP_SPLINE_TILE_LDS_BYTES: one
 *            persistent workgroup per compute unit stages the whole weight tensor into LDS once and reads it from there.
 *            Measured slower than global from 4 096 edges on, 2.5 times at 1 M (one wave per SIMD), hence
 *            never the rule's choice.
 * Both give the same bits.  `flags`: PYG_HIP_SPLINE_FORCE_LDS / _GLOBAL (tests, measurements; a forced lds call whose weights
 * do not fit runs global).  pyg_hip_spline_last_route() names what the last weighting call of this thread
 * ran: "<forward|backward_x|backward_basis> <lds|global> tx<lanes per edge> te<edges per tile>".  An edge whose rows exceed
 * the LDS tile (PYG_HIP_SPLINE_TILE_EDGE_BYTES; thousands of channels): PYG_HIP_ERR_UNSUPPORTED.
 *
 * backward_weight: the E * S pair positions are stably sorted by weight index (pyg_hip_index_sort's kernels; an index outside
 * [0, K) is keyed K, a bucket nobody reads), one workgroup finds the row starts, one launch deals (weight, chunk of
 * PYG_HIP_SPLINE_TILE_CHUNK consecutive sorted pairs, 64 x 64 tile of the matrix) work items whose threads keep their sums in
 * registers; a weight of one chunk is written straight to grad_weight, a longer one through per-chunk slabs in the workspace
 * that a second launch adds in chunk order; weights without pairs are written as zeros (no memset).  `flags` bits 8 .. 12:
 * log2 of the chunk of this call, 9 .. 12 (0: the constant; a measurement hook -- the bits of long weights depend on it).
 *
 * A weight_index outside [0, K) never causes an access outside a buffer: the pair contributes nothing and a pinned word of the
 * device is set -- no operator here synchronises --: the NEXT pyg_hip_spline_* call on that device fails with
 * PYG_HIP_ERR_INVALID, and pyg_hip_spline_pending_error() returns and clears the word (meaningful once the stream has been
 * synchronised).  Workspaces: the sizes below, 16-byte aligned; less is PYG_HIP_ERR_WORKSPACE.
 */
#define PYG_HIP_SPLINE_FORCE_LDS 1
#define PYG_HIP_SPLINE_FORCE_GLOBAL 2
#define PYG_HIP_SPLINE_FORCE_MASK 3
#define PYG_HIP_SPLINE_ROUTE_UNSUPPORTED 0
#define PYG_HIP_SPLINE_ROUTE_LDS 1
#define PYG_HIP_SPLINE_ROUTE_GLOBAL 2
#define PYG_HIP_SPLINE_TILE_LDS_BYTES 0       /* route lds: the weight tensor fits this many bytes of LDS */
#define PYG_HIP_SPLINE_TILE_CHUNK 1           /* backward_weight: sorted pairs per work item */
#define PYG_HIP_SPLINE_TILE_EDGE_BYTES 2      /* LDS of the edge tile */
#define PYG_HIP_SPLINE_TILE_DW 3              /* backward_weight: side of a work item's matrix tile */
PYG_HIP_API int pyg_hip_spline_route(int dtype, int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K);
PYG_HIP_API const char* pyg_hip_spline_last_route(void);
PYG_HIP_API int pyg_hip_spline_tile(int which);
PYG_HIP_API int pyg_hip_spline_pending_error(void);
PYG_HIP_API int pyg_hip_spline_basis(int dtype, const void* pseudo, const int64_t* kernel_size, const uint8_t* is_open_spline,
                                     int64_t E, int64_t D, int degree, void* basis, int64_t* weight_index, void* stream);
PYG_HIP_API int pyg_hip_spline_basis_backward(int dtype, const void* grad_basis, const void* pseudo, const int64_t* kernel_size,
                                              const uint8_t* is_open_spline, int64_t E, int64_t D, int64_t S, int degree,
                                              void* grad_pseudo, void* stream);
PYG_HIP_API int pyg_hip_spline_weighting(int dtype, const void* x, const void* weight, const void* basis, const int64_t* weight_index,
                                         int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K, int flags, void* out,
                                         void* stream);
PYG_HIP_API size_t pyg_hip_spline_backward_x_workspace_size(int dtype, int64_t M_in, int64_t M_out, int64_t K);
PYG_HIP_API int pyg_hip_spline_weighting_backward_x(int dtype, const void* grad_out, const void* weight, const void* basis,
                                                    const int64_t* weight_index, int64_t E, int64_t S, int64_t M_in, int64_t M_out,
                                                    int64_t K, int flags, void* workspace, size_t workspace_bytes, void* grad_x,
                                                    void* stream);
PYG_HIP_API int pyg_hip_spline_weighting_backward_basis(int dtype, const void* grad_out, const void* x, const void* weight,
                                                        const int64_t* weight_index, int64_t E, int64_t S, int64_t M_in,
                                                        int64_t M_out, int64_t K, int flags, void* grad_basis, void* stream);
PYG_HIP_API size_t pyg_hip_spline_backward_weight_workspace_size(int dtype, int64_t E, int64_t S, int64_t M_in, int64_t M_out,
                                                                 int64_t K, int flags);
PYG_HIP_API int pyg_hip_spline_weighting_backward_weight(int dtype, const void* grad_out, const void* x, const void* basis,
                                                         const int64_t* weight_index, int64_t E, int64_t S, int64_t M_in,
                                                         int64_t M_out, int64_t K, int flags, void* workspace,
                                                         size_t workspace_bytes, void* grad_weight, void* stream);

/* ---- graclus_cluster: greedy matching in random order, in parallel rounds --------------------------------------------
 *
 * Replaces pyg::graclus_cluster (schema ops/graclus.cpp; CPU ops/cpu/graclus_kernel.cpp; CUDA ops/cuda/graclus_kernel.cu).
 * rowptr [N + 1] and col [E]: int64 CSR on the device; weight [E] in `weight_dtype` (PYG_F32 / F64 / F16 / BF16; 16-bit
 * weights are widened exactly for the comparisons) or NULL with weight_dtype PYG_HIP_GRACLUS_NO_WEIGHT; perm [N]: int64, a
 * permutation of 0 .. N-1; out [N]: int64.  N < 2^31 (PYG_HIP_ERR_UNSUPPORTED otherwise).
 *
 * The operator is the reference's sequential CPU loop: with out = -1 everywhere, visit u = perm[0], perm[1], ...; a node with
 * out[u] >= 0 is skipped; otherwise
 *   without weights  u takes the first entry x of its row, in CSR order, with x != u and out[x] < 0;
 *   with weights     u takes, among the entries x with out[x] < 0 and weight >= 0, the one of the largest weight, the LAST one
 *                    among equals (NaN and negative weights never win, -0.0 and +inf do; a self loop can win, then u stays alone);
 * and out[u] = out[x] = min(u, x), or out[u] = u when there is no such entry.
 *
 * Every route computes exactly that in rounds.  rank = the inverse of perm.  A node is active while out[u] < 0.  A candidate of
 * an active u is a row entry x with out[x] < 0 and (without weights) x != u, (with weights) weight >= 0.  Per round:
 *   phase A  every active u offers rank(u) to m[x] of every candidate x and to m[u]; m[.] is the minimum of the round's offers
 *            (an integer maximum of `round * 2^32 + (2^32 - 1 - rank)`: no clearing, no dependence on thread order); u records
 *            its pick p(u) by the rule above, or none;
 *   phase B  u is ready iff rank(u) == m[u] and (p(u) is none or rank(u) == m[p(u)]); a ready u writes out[u] = out[p] =
 *            min(u, p), or out[u] = u without a pick.  The others wait for the next round.
 * A ready u is the earliest node that can still reach u or p(u), so what it sees is what the sequential visit sees at u; two ready
 * nodes never share a node, so phase B has no write conflict; the active node of the smallest rank is always ready, so at most N
 * rounds run.  The round count is a function of the input alone: the same on every route and in tests/_graclus_ref.py.
 *
 * Routes.  pyg_hip_graclus_route(N, E, flags) answers, without touching a device, which route a call takes
 * (PYG_HIP_GRACLUS_ROUTE_*; 0 for N or E negative or N >= 2^31):
 *   single   N <= PYG_HIP_GRACLUS_TILE_SINGLE_NODES and E <= PYG_HIP_GRACLUS_TILE_SINGLE_EDGES: ONE launch of one workgroup of
 *            PYG_HIP_GRACLUS_TILE_SINGLE_THREADS threads that strides over the nodes in both phases, a workgroup barrier between
 *            them; it counts the nodes still active itself.  No host read: capturable into a graph.
 *   multi    two launches per round over all nodes (PYG_HIP_GRACLUS_TILE_MULTI_THREADS threads per workgroup), enqueued in
 *            batches of PYG_HIP_GRACLUS_TILE_BATCH rounds.  Phase B subtracts what it matched from the round's word of active
 *            nodes (one integer atomic per workgroup); every launch returns at once when the previous round's word is zero.
 *            After each batch the host reads the word back through pinned memory -- the call SYNCHRONISES the stream, once per
 *            batch -- and enqueues another batch if nodes are left.  No grid barrier, no cooperative launch, no spinning.
 * PYG_HIP_GRACLUS_FORCE_SINGLE / _MULTI override the rule (tests, measurements); a forced single call above the capacity
 * (PYG_HIP_GRACLUS_TILE_SINGLE_MAX_NODES nodes or _SINGLE_MAX_EDGES edges) runs multi.  The rule's thresholds are the measured
 * cross-over.  pyg_hip_graclus_last_route() names what the last call of this thread ran:
 * "<single|multi> r<rounds> b<read-backs>" (single: the rounds come from a pinned word the kernel writes, so the text is
 * meaningful once the stream has been synchronised; its read-backs are 0), "none r0 b0" for N == 0.
 * pyg_hip_graclus_tile(which) returns the constants.  workspace: pyg_hip_graclus_workspace_size(N, E, flags) bytes, 16-byte
 * aligned (32-bit state, rank and pick and the 64-bit m of every node).
 *
 * Bad input never causes an access outside a buffer: a col entry outside [0, N) is no candidate and forms no address, a row
 * range is clamped into [0, E], a perm entry outside [0, N) is dropped and a node whose rank nobody wrote (a repeated entry)
 * is ranked behind all others.  Any of these sets a pinned word of the device: the NEXT pyg_hip_graclus call on that device
 * fails with PYG_HIP_ERR_INVALID, and pyg_hip_graclus_pending_error() returns and clears the word (meaningful once the stream
 * has been synchronised).  The result of such a call is unspecified, but every out[u] is written.
 */
#define PYG_HIP_GRACLUS_NO_WEIGHT (-1)
#define PYG_HIP_GRACLUS_FORCE_SINGLE 1
#define PYG_HIP_GRACLUS_FORCE_MULTI 2
#define PYG_HIP_GRACLUS_FORCE_MASK 3
#define PYG_HIP_GRACLUS_ROUTE_UNSUPPORTED 0
#define PYG_HIP_GRACLUS_ROUTE_SINGLE 1
#define PYG_HIP_GRACLUS_ROUTE_MULTI 2
#define PYG_HIP_GRACLUS_TILE_SINGLE_NODES 0     /* single: the rule takes it up to this many nodes ... */
#define PYG_HIP_GRACLUS_TILE_SINGLE_EDGES 1     /* ... and this many edges */
#define PYG_HIP_GRACLUS_TILE_SINGLE_THREADS 2   /* single: threads of the one workgroup */
#define PYG_HIP_GRACLUS_TILE_SINGLE_MAX_NODES 3 /* a forced single call runs multi above this many nodes */
#define PYG_HIP_GRACLUS_TILE_MULTI_THREADS 4    /* multi: threads per workgroup, one node each */
#define PYG_HIP_GRACLUS_TILE_BATCH 5            /* multi: rounds enqueued between two read-backs */
#define PYG_HIP_GRACLUS_TILE_SINGLE_MAX_EDGES 6 /* ... or above this many edges */
PYG_HIP_API int pyg_hip_graclus_route(int64_t N, int64_t E, int flags);
PYG_HIP_API const char* pyg_hip_graclus_last_route(void);
PYG_HIP_API int pyg_hip_graclus_tile(int which);
PYG_HIP_API size_t pyg_hip_graclus_workspace_size(int64_t N, int64_t E, int flags);
PYG_HIP_API int pyg_hip_graclus(const int64_t* rowptr, const int64_t* col, int weight_dtype, const void* weight, const int64_t* perm,
                                int64_t N, int64_t E, int flags, void* workspace, size_t workspace_bytes, int64_t* out, void* stream);
PYG_HIP_API int pyg_hip_graclus_pending_error(void);

/* ---- measurement hooks (bench.py) --------------------------------------------------------- */

/*
 * CSR reductions.  src viewed as [leading, E, K]; indptr holds rows + 1 ascending offsets per slice,
 * `indptr_slice_stride` elements apart (0: one indptr shared by all slices, read in place);
 * out / arg_out [leading, rows, K].  Replaces pyg::segment_{sum,mean,min,max}_csr (schemas
 * ops/segment_csr.cpp:153-172; CPU ops/cpu/segment_csr_kernel.cpp:32-536; CUDA
 * ops/cuda/segment_csr_kernel.cu).
 *   op 0 sum : every row adds src[slice, indptr[r] .. indptr[r+1]) to the CURRENT contents of its out
 *              slot (the caller zero-fills a fresh output; a caller-supplied `out` accumulates)
 *   op 1 mean: out = row sum / max(row length, 1), previous contents ignored; floating dtypes only
 *   op 2 min / 3 max: strict < / >, first match; fresh == 0: the running state starts from the current contents
 *              of `out`; fresh != 0: from numeric_limits max() / lowest() WITHOUT reading `out` (it need not be
 *              pre-filled; ABI <= 7 read it and wanted pyg_hip_fill_reduce_identity first -- still harmless), and rows
 *              without a contribution are reset to 0.  arg_out receives the winning source position or the
 *              sentinel E for EVERY slot (it need not be pre-filled either).
 * Rows are reduced in source order in the reference's opmath, so results are bit-identical to the CPU
 * kernel for every dtype unless rows are long and few (then lanes split a row) or longer than 512
 * positions per lane (4096 for rows narrower than 64 bytes: hub rows, see pyg_hip_segment_csr_ws); floating
 * sums of such rows differ by rounding, min/max/arg stay exact, and every run gives the same bits.
 * Non-finite values and signed zeros, the same on every row kernel, lane-split, hub or not: strict
 * compares -- a NaN in `src` never wins, a NaN / -0 / identity in a caller's `out` slot stays with arg = E unless strictly
 * beaten, +0 and -0 tie and the first position wins; {+Inf, -Inf} or a NaN make a sum / mean NaN; -0 + {-0, ...} stays -0.
 */
PYG_HIP_API int pyg_hip_segment_csr(int op, int dtype, const void* src, const int64_t* indptr,
                                    int64_t indptr_slice_stride, void* out, int64_t* arg_out, int fresh,
                                    int64_t leading, int64_t rows, int64_t E, int64_t K, void* stream);

/*
 * The same with scratch for HUB rows.  The row kernels give a row to 1 / 8 / 64 lanes; a row of more than 512 positions per
 * lane (a power-law graph's popular destination) is skipped there.  Without scratch a second launch gives every such row to
 * ONE workgroup (~9 GB/s per row: a row holding 2.5 % of 8 M positions of 256 bytes then takes 6 ms of a 0.5 ms call).
 * With `workspace` (pyg_hip_csr_hub_workspace_size() bytes of device memory, contents irrelevant, not kept) the skipped rows
 * are registered there in chunks of 2048 positions, a second launch deals the chunks to all workgroups, and a third
 * combines the chunks' partial results of a row in chunk order: no float atomics, the same bits on
 * every run; sums of hub rows differ from the sequential order by rounding (like the lane-split rows), min / max / arg
 * stay exact.  A smaller workspace is legal: the chunk length doubles until the partial results fit, too small means "without".
 * pyg_hip_csr_hub_workspace_size: op 0 ... 3 as above, 4 = gather_csr; 0 when no row can be a hub (leading * E <= 512).
 */
PYG_HIP_API size_t pyg_hip_csr_hub_workspace_size(int op, int dtype, int64_t leading, int64_t E, int64_t K);
PYG_HIP_API int pyg_hip_segment_csr_ws(int op, int dtype, const void* src, const int64_t* indptr,
                                       int64_t indptr_slice_stride, void* out, int64_t* arg_out, int fresh,
                                       int64_t leading, int64_t rows, int64_t E, int64_t K, void* workspace,
                                       size_t workspace_bytes, void* stream);

/*
 * out[slice, e, :] = src[slice, r, :] for every position e of row r; positions covered by no row keep
 * their contents.  src [leading, rows, K], out [leading, E, K].  Replaces pyg::gather_csr (schema
 * ops/segment_csr.cpp:170-172; CPU ops/cpu/segment_csr_kernel.cpp:551-648).
 */
PYG_HIP_API int pyg_hip_gather_csr(int dtype, const void* src, const int64_t* indptr,
                                   int64_t indptr_slice_stride, void* out, int64_t leading, int64_t rows,
                                   int64_t E, int64_t K, void* stream);
/* ... with scratch for hub rows (pyg_hip_csr_hub_workspace_size(4, ...)): their positions are written by all workgroups. */
PYG_HIP_API int pyg_hip_gather_csr_ws(int dtype, const void* src, const int64_t* indptr,
                                      int64_t indptr_slice_stride, void* out, int64_t leading, int64_t rows,
                                      int64_t E, int64_t K, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Softmax over the groups ptr[g] .. ptr[g+1] along the middle axis of src [outer, D, inner], per
 * (group, outer, inner) head; `out` must be zero-filled by the caller (positions outside every group
 * stay 0).  float32 / float64.  Replaces pyg::softmax_csr / pyg::softmax_csr_backward (schemas
 * ops/softmax.cpp:46-53; CPU only in the reference: ops/cpu/softmax_kernel.cpp:58-222).
 * The maximum starts from lowest(), not -Inf: a -Inf logit gives exactly 0 and the softmax of the rest;
 * a group of -Inf only, or with a +Inf or a NaN, is NaN in that group and head only; a one-element group is exactly 1.
 */
PYG_HIP_API int pyg_hip_softmax_csr(int dtype, const void* src, const int64_t* ptr, void* out, int64_t outer,
                                    int64_t D, int64_t inner, int64_t groups, void* stream);
PYG_HIP_API int pyg_hip_softmax_csr_backward(int dtype, const void* out, const void* out_grad,
                                             const int64_t* ptr, void* in_grad, int64_t outer, int64_t D,
                                             int64_t inner, int64_t groups, void* stream);

/*
 * What a CSR call is made of -- segment_csr, gather_csr, softmax_csr and its backward, and the rows back end of pyg_hip_scatter
 * (csr_rows / sort_rows) and of the COO operators.  pyg_hip_csr_route asks, pyg_hip_csr_last_route tells, as
 *   '<segment|gather|softmax|softmax_bwd> <kernel> v<V> <none|long|chunks|chunks+combine>[ ch<CH>]'
 * or 'none' (an empty call: leading x rows x K == 0, for gather and softmax also E == 0) or 'unsupported' (integer mean, softmax
 * of a dtype other than float32 / float64, an unknown family or dtype, a negative size).
 *   family   0 ... 3 the reductions, 4 gather_csr, 5 / 6 softmax_csr / its backward with leading = outer, rows = groups, E = D,
 *            K = inner
 *   flags    bit 0: the rows are read through a permutation (the sort-based scatter)
 *   misalign bits 0 ... 3: the low four bits of (src | out); bits 8 ... 15: the low eight bits of the scratch's address
 *   num_cus  compute units of the device; 0: the current device's.  With num_cus > 0 the query needs no device.
 * With avg = leading x E / (leading x rows) positions per row and rows of K x sizeof(dtype) bytes:
 *   V        16 / sizeof(dtype) when rows are whole 16-byte slices and src and out are 16-byte aligned (never softmax, never
 *            the stream kernel), else 1: elements per thread.  items = leading x rows x K / V.
 *   kernel   the first line that applies
 *     stream   rows of at most 16 elements and less than 64 bytes, 12 <= avg < 64, V == 1; not gather, not through a
 *              permutation; softmax: rows of less than 32 bytes and avg >= 33 (backward: 12).  LDS-streamed, a thread per
 *              (row, element)
 *     lanes64  rows of less than 64 bytes, avg >= 256                     64 lanes over the positions of an item
 *     lanes8   rows of less than 64 bytes, avg >= 64                      8 lanes
 *     narrow8  rows of 16, 32 or 48 bytes, avg >= 16                      8 lanes
 *     lanes64  avg >= 1024 and items x 8 < num_cus x 2048
 *     lanes8   avg >= 64 and items < num_cus x 2048
 *     narrow8  gather only: rows of less than 64 bytes, avg >= 8 (V > 1) or avg >= 32 (V == 1)
 *     row1     everything else: one lane per item, the reference's order of operations
 *   hub rows rows of more than cut = 512 x lanes positions (stream: 4096) are skipped by the row kernel.  None can exist when
 *            E <= cut or there is one row (softmax: one group) only: 'none'.  Else
 *     long            no scratch, scratch too small, softmax: a second launch gives every hub row to one workgroup
 *     chunks          scratch (pyg_hip_csr_hub_workspace_size; from its first 256-byte boundary on): hub rows are registered
 *                     in chunks of CH = 2048 positions -- doubled until the partial results fit the scratch -- that a second
 *                     launch deals to all workgroups.  gather, and reductions with E <= CH (every hub is one chunk)
 *     chunks+combine  reductions with E > CH: a third launch combines the chunks' partial results of a row in chunk order
 * pyg_hip_csr_route launches nothing and returns a string of the calling thread's that the next query overwrites;
 * pyg_hip_csr_last_route names the last CSR launch made on the calling thread ('none' before the first).
 */
PYG_HIP_API const char* pyg_hip_csr_route(int family, int dtype, int64_t leading, int64_t rows, int64_t E, int64_t K,
                                          int flags, size_t workspace_bytes, unsigned misalign, int num_cus);
PYG_HIP_API const char* pyg_hip_csr_last_route(void);

/*
 * Device hash map key -> first position: the kernels behind torch.classes.pyg.CUDAHashMap
 * (pyg_lib/csrc/classes/cuda/hash_map.cu:36-100, a cuco::static_map wrapper in the reference).
 * The table is caller-owned: `slots` = pyg_hip_hash_map_slots(n, load_factor) entries (a power of two)
 * of table_keys (uint64) and table_vals (int64).  Keys are int16 / int32 / int64 (widened with sign extension).
 * `build` leaves the number of distinct keys in *distinct_dev (device memory); duplicate keys map to their first
 * position.  `get` writes the position or -1 per query.
 *
 * INT64_MIN is reserved: it marks an empty slot, as cuco's empty-key sentinel does in the reference.  `build` skips a
 * key equal to it -- the key touches neither table array and is not counted in *distinct_dev, the positions of the
 * other keys are unchanged -- and `get` answers -1 for it on every table.  (The minima of int16 and int32 widen to other
 * values and are ordinary keys.)
 *
 * pyg_hip_hash_map_slots: the smallest power of two >= 16 that is >= max(n, 1) / load_factor + 1, so at least one slot
 * stays empty; a load factor outside (0, 1] counts as 0.5.  -1 if n < 0 or if no power of two below 2^62 is large enough
 * (a denormal load factor).  build / get return PYG_HIP_ERR_INVALID, before anything is launched, for a dtype other than
 * the three above, `slots` that is no power of two or (build) not greater than n, and NULL arrays.
 */
PYG_HIP_API int64_t pyg_hip_hash_map_slots(int64_t n, double load_factor);
PYG_HIP_API int pyg_hip_hash_map_build(int key_dtype, const void* keys, int64_t n, uint64_t* table_keys,
                                       int64_t* table_vals, int64_t slots, int64_t* distinct_dev, void* stream);
PYG_HIP_API int pyg_hip_hash_map_get(int key_dtype, const void* query, int64_t m, const uint64_t* table_keys,
                                     const int64_t* table_vals, int64_t slots, int64_t* out, void* stream);

/* When enabled (per calling thread), every dominant-kernel launch is bracketed by a pair of HIP
 * events recorded on the stream the kernel is launched on.  pyg_hip_profile_collect waits for the
 * recorded launches, writes up to `capacity` durations (milliseconds, launch order) and returns
 * how many launches were recorded since the last collect. */
PYG_HIP_API void pyg_hip_profile_enable(int on);
PYG_HIP_API int pyg_hip_profile_collect(float* ms_out, int capacity);

/* Hand-written device-to-device streaming copy of `bytes` bytes (16-byte aligned buffers), the yardstick
 * bench.py prints as roofline.achievable: mode 0 = fine-grained non-persistent sweep (the best copy found on
 * this hardware), 1 = persistent with one contiguous range per workgroup, 2 = persistent cyclic -- the two
 * segment_matmul tile schedules without the arithmetic.  Measurement support; no operator calls it. */
PYG_HIP_API int pyg_hip_stream_copy(const void* src, void* dst, size_t bytes, int mode, void* stream);

/* The shader clock the chip actually runs at while other streams load it: one wave on `stream` watches the shader-clock
 * counter and the constant 100 MHz counter for `milliseconds` and leaves {shader cycles, 100 MHz ticks} in out2 (device
 * memory, 2 x uint64): MHz = out2[0] / out2[1] * 100.  The fp32 MFMA peak of the data sheet (157 TFLOP/s) is quoted at
 * 2.4 GHz; under a sustained MFMA + HBM load the chip clocks lower, and bench.py prices the fp32 kernel against both. */
PYG_HIP_API int pyg_hip_clock_probe(uint64_t* out2, double milliseconds, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PYG_HIP_H_ */
