/* kvc.h — C-ABI of the MI355X (gfx950) KV-cache compression hot path.
 *
 * Drop-in boundary for ONE path of assassin808/KVCache-Factory (reference @ 2025-02-18): the
 * post-prefill scoring + eviction step behind `kv_cluster.update_kv(key_states, query_states,
 * value_states, attention_mask, num_key_value_groups)`:
 *     SnapKVCluster.update_kv          pyramidkv/pyramidkv_utils.py:306-347
 *     PyramidKVCluster.update_kv       pyramidkv/pyramidkv_utils.py:197-283
 *     H2OKVCluster.update_kv           pyramidkv/pyramidkv_utils.py:533-575
 *     StreamingLLMKVCluster.update_kv  pyramidkv/pyramidkv_utils.py:595-620
 * The reference has no C/FFI interface on this path (it is ~60 lines of torch ops per method);
 * these entry points are what a ctypes binding of `update_kv` binds (INTEGRATION.md shows the
 * stub).  Implemented in kvcache_factory_amd/csrc/ (hand-written HIP, libkvc_hip.so).
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer (HBM), 16-byte aligned; nothing is copied to the host;
 *   - the library never allocates device memory, never synchronises the stream and never throws:
 *     all kernels are enqueued on `hip_stream` (a hipStream_t, NULL = default stream);
 *   - tensors are indexed [b][h][l][d] with d contiguous and element strides given in the params;
 *   - outputs: k_out/v_out [bsz][n_q_heads][k+window][head_dim] in the input dtype, dense or with a caller-chosen
 *     head stride (kvc_params.out_stride_h: a decode cache with spare rows per head),
 *     idx_out [bsz][n_q_heads][k] int64 (value-descending order, like torch.topk), scores_out
 *     [bsz][n_q_heads][q_len-window] in the input dtype (the pooled scores of :328-333);
 *   - return value 0 on success, negative kvc_status otherwise; kvc_last_error() gives the text.
 */
#ifndef KVC_H_
#define KVC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KVC_VERSION 5

typedef enum kvc_status {
    KVC_OK = 0,
    KVC_ERR_INVALID = -1,      /* the reference would assert / raise (pyramidkv_utils.py:289,309,333) */
    KVC_ERR_UNSUPPORTED = -2,  /* valid for the reference, not implemented by this library (documented limits) */
    KVC_ERR_WORKSPACE = -3,    /* workspace missing, misaligned or smaller than kvc_workspace_bytes() */
    KVC_ERR_ALIGNMENT = -4,    /* a pointer or stride is not 16-byte aligned */
    KVC_ERR_HIP = -5           /* a HIP runtime call failed (message carries hipGetErrorString) */
} kvc_status;

typedef enum kvc_method {      /* which update_kv is being replaced */
    KVC_SNAPKV = 0,            /* pyramidkv_utils.py:306-347 */
    KVC_PYRAMIDKV = 1,         /* :197-283 — same kernels, caller passes the per-layer k (kvc_pyramid_k) */
    KVC_H2O = 2,               /* :533-575 — all q_len query rows, no pooling */
    KVC_STREAMINGLLM = 3,      /* :595-620 — no scoring: first k + last window tokens */
    KVC_ADAKV = 4,             /* :622-757 — window-MEAN scores, per-head budgets from a global top-(H*base), ragged cache:
                                  kvc_ragged_* entry points only (k = base capacity = max_capacity_prompt - W) */
    KVC_HEADKV = 5,            /* :760-878 — the same with per-head budgets given by the caller */
    KVC_L2NORM = 6             /* :394-429 — L2NormCluster: the k smallest-norm keys per head, ascending; no query, no window:
                                  kvc_l2norm_* entry points only (k = rows kept = max_capacity_prompt) */
} kvc_method;

typedef enum kvc_dtype { KVC_BF16 = 0, KVC_FP16 = 1, KVC_FP32 = 2 } kvc_dtype;
typedef enum kvc_pooling { KVC_POOL_NONE = 0, KVC_POOL_AVG = 1, KVC_POOL_MAX = 2 } kvc_pooling;

typedef enum kvc_tie_mode {
    KVC_TIES_TORCH_CPU = 0,    /* membership and order of equal scores exactly as torch-CPU topk
                                  (libstdc++ partial_sort when k*64<=n, else nth_element+sort) */
    KVC_TIES_CANONICAL = 1     /* value descending, index ascending (fast path) */
} kvc_tie_mode;

typedef enum kvc_dot_mode {
    KVC_DOT_EXACT = 0,         /* window QK^T as the d-ascending fp32 fmaf chain (f32-input MFMA): bit-identical to the CPU
                                  oracle, and the arithmetic the reference's fp16/fp32 GEMM was measured to use */
    KVC_DOT_MFMA16 = 1         /* packed bf16/fp16 16-deep MFMA (16x less matrix time; fp32 inputs fall back to EXACT).
                                  Tolerance mode: a logit may differ from EXACT by 1 unit in the last place (~1e-4 of
                                  the entries), which can move a candidate across the top-k threshold.  H2O: two
                                  recomputing passes with no logit matrix (workspace: two floats per query row), hardware
                                  exp and fp32 sums in tile order — pooled scores within 1 unit in the last place. */
} kvc_dot_mode;

typedef struct kvc_params {
    int32_t method;            /* kvc_method */
    int32_t dtype;             /* kvc_dtype of q, k, v and of every non-index output */
    int32_t bsz;               /* batch (the reference runs bsz = 1, README.md:29; code is batch-agnostic) */
    int32_t n_q_heads;         /* heads of q and of the outputs (32 for Llama-3-8B / Mistral-7B) */
    int32_t n_kv_heads;        /* heads present in k and v: n_q_heads when the caller passes the
                                  repeat_kv()-expanded tensors like the reference (llama_model.py:277-278),
                                  or the model's KV heads (8) to read each KV head once.  Query head h
                                  reads kv head h / (n_q_heads / n_kv_heads). */
    int32_t q_len;             /* L: key_states.shape[-2] == query_states.shape[-2] (:309) */
    int32_t head_dim;          /* D: 64 or 128 */
    int32_t window;            /* W = window_size: the last W queries score, the last W tokens are kept */
    int32_t k;                 /* prefix tokens kept per head: max_capacity_prompt - W (:334), or the
                                  PyramidKV per-layer budget (:214); 0 <= k <= L - W */
    int32_t kernel_size;       /* pooling kernel (odd; padding = kernel_size/2, stride 1) (:328-333) */
    int32_t pooling;           /* kvc_pooling; ignored for H2O (no pooling, :555-561) and StreamingLLM */
    int32_t tie_mode;          /* kvc_tie_mode */
    int32_t debug_stage_mask;  /* testing / profiling aid, 0 in production.  Bits 0-2 (kvc_scores, kvc_compress_batch): only the
                                  scoring kernels named by bit0 = K-scan (logits), bit1 = row-sum, bit2 = pool are
                                  enqueued; kvc_compress requires them 0.  Bit3 / bit4: force the two-kernel / the
                                  one-workgroup-per-head form of the softmax+pool stage (identical results; the
                                  library picks by the number of heads x items otherwise).  Bit5 / bit6
                                  (kvc_compress_batch, timing only): skip the scoring kernels / skip scoring and selection
                                  and reuse what the previous identical call left in the workspace and the outputs.  Bit7
                                  (H2O exact mode, testing): hold 512 query rows of the logit matrix at a time instead of
                                  as many as fit in 1 GiB (identical results).  Bit8 (measurement): the softmax stage reloads the
                                  logits in its second pass instead of keeping the exponentials in registers (identical results).
                                  Bit9 (measurement): G * W == 128 query rows per KV head scanned by the one-M-tile-at-a-time
                                  kernel instead of the four-waves-share-a-tile one (identical results).  Bit10 (measurement): at window 8 the
                                  one-workgroup-per-head softmax stage without its chain-wave / worker-wave split (identical results).
                                  Bit11 (H2O exact mode, testing): round 2's kernels that write the logit matrix to the
                                  workspace instead of the fused one that keeps 16 query rows of it in registers (identical results).
                                  Bit12 (measurement): at windows 16 / 32 / 64 the one-workgroup-per-head softmax stage that reads the
                                  logits twice instead of the 16-rows-per-workgroup form that reads them once (identical results).
                                  Bit13 (testing): tie_mode torch_cpu with every budget in the one-wave heap's regime (16-bit,
                                  1 <= k <= 128, k * 64 <= q_len - window): the separate selection and gather launches instead of
                                  the kernel that copies K / V rows as the selection finalises them (identical results).
                                  Bit14 (measurement): the window-8 stage with its exponentials kept in registers, one workgroup
                                  per CU, instead of the form that recomputes them in its second pass so that two heads share a
                                  CU (identical results). */
    int32_t dot_mode;          /* kvc_dot_mode */
    int64_t q_stride_b, q_stride_h, q_stride_l;   /* element strides of q[b][h][l][:] */
    int64_t k_stride_b, k_stride_h, k_stride_l;
    int64_t v_stride_b, v_stride_h, v_stride_l;
    int64_t out_stride_h;      /* elements between consecutive heads of k_out / v_out ([b][h_q][row][D], rows dense).
                                  0 = dense, (k + window) * head_dim.  Larger: the caller's decode cache with spare rows
                                  per head ([b][h_q][capacity][D]) — K' / V' are written straight into their final home
                                  (the reference cats them into a fresh tensor, llama_model.py:286).  A multiple of 8
                                  (16-bit) or 4 (fp32) elements, >= (largest k + window) * head_dim. */
} kvc_params;

/* Library / ABI version (== KVC_VERSION). */
int kvc_version(void);

/* Thread-local text of the last error returned on this thread ("" if none). */
const char* kvc_last_error(void);

/* Bytes of device scratch kvc_compress / kvc_scores / kvc_select need for these params
 * (0 for StreamingLLM).  Returns 0 and sets the error text if the params are invalid. */
size_t kvc_workspace_bytes(const kvc_params* p);

/* The whole update_kv: scores (A1-A5, or A10 for H2O) -> per-head top-k (A7) -> gather + window
 * tail (A8), for the method in p->method.  Replaces the body of
 *   SnapKVCluster.update_kv :317-346 / PyramidKVCluster.update_kv :220-283 /
 *   H2OKVCluster.update_kv :544-575 / StreamingLLMKVCluster.update_kv :607-620.
 * q: query tensor base: row l of head h is read at q + b*q_stride_b + h*q_stride_h + l*q_stride_l.  SnapKV / PyramidKV
 *    dereference rows L-W .. L-1 ONLY, so a caller that kept just the window rows ([b][h][W][D], as a layer-batching
 *    host does) passes window_base - (L-W)*q_stride_l; H2O reads every row; StreamingLLM ignores q (may be NULL).
 * idx_out and scores_out may be NULL (scores_out is never written for StreamingLLM). */
int kvc_compress(const kvc_params* p, const void* q, const void* k, const void* v,
                 void* k_out, void* v_out, int64_t* idx_out, void* scores_out,
                 void* workspace, size_t workspace_bytes, void* hip_stream);

/* Batched form: n_items independent update_kv calls of IDENTICAL shape/dtype/strides (described by *p; p->k is
 * ignored) and per-item budgets k_per_item[i] — e.g. the 32 layers of one prompt (the reference runs them as 32
 * sequential calls, llama_model.py:285; no call reads another's result, and the prefill attention of every layer runs
 * on the UNcompressed K/V, llama_model.py:306-313, so a host may collect the layers and compress them after the last
 * one).  Every kernel is launched once per chunk of 32 items (n_items may be larger; chunks reuse the workspace), so the
 * small per-call kernels stop being launch-latency bound.  The arrays are HOST arrays of DEVICE
 * pointers (they are copied into the kernel arguments; nothing is staged on the device).  idx_out / scores_out may be
 * NULL, as may their entries.  Results are identical to n_items kvc_compress calls.
 * out_stride_h_per_item: NULL (every item uses p->out_stride_h) or n_items head strides in elements, one per item,
 * 0 = dense — each layer's decode cache sized for its own budget (PyramidKV's layers differ by 14x at 8k).
 * Workspace: kvc_workspace_bytes_batch(). */
size_t kvc_workspace_bytes_batch(const kvc_params* p, int n_items, const int32_t* k_per_item);
int kvc_compress_batch(const kvc_params* p, int n_items, const int32_t* k_per_item,
                       const void* const* q, const void* const* k, const void* const* v,
                       void* const* k_out, void* const* v_out, int64_t* const* idx_out, void* const* scores_out,
                       const int64_t* out_stride_h_per_item,
                       void* workspace, size_t workspace_bytes, void* hip_stream);

/* Stage entry points (same kernels kvc_compress enqueues), exposed so parity can be pinned stage by stage. */

/* A1-A5 (A10 for H2O): pooled scores [bsz][n_q_heads][L-W] in dtype (:317-333 / :544-561). */
int kvc_scores(const kvc_params* p, const void* q, const void* k, void* scores_out,
               void* workspace, size_t workspace_bytes, void* hip_stream);

/* A7: idx_out[b][h][0..k) = topk(scores[b][h][0..L-W), k).indices (:334).
 * Workspace: kvc_select_workspace_bytes(p) bytes, 256-byte aligned (0 for most shapes: only tie_mode torch_cpu in its
 * nth_element regime, k*64 > L-W, keeps position lists — and arrays that do not fit in LDS — there). */
size_t kvc_select_workspace_bytes(const kvc_params* p);
int kvc_select(const kvc_params* p, const void* scores, int64_t* idx_out,
               void* workspace, size_t workspace_bytes, void* hip_stream);

/* A8 for one tensor: out[b][h] = cat(src[b][h/g][idx[b][h][:]], src[b][h/g][L-W:]) (:341-346).
 * idx == NULL means idx[t] = t (StreamingLLM, :607-608).  Strides are those of `src`. */
int kvc_gather(const kvc_params* p, const void* src, int64_t stride_b, int64_t stride_h, int64_t stride_l,
               const int64_t* idx, void* out, void* hip_stream);

/* PyramidKV per-layer budget, host arithmetic only (:205-215, beta = 20 at :174).
 * Returns the k for `layer_idx`; -1 means "pass-through" (q_len < cap, :218). */
int64_t kvc_pyramid_k(int64_t max_capacity_prompt, int64_t window, int64_t q_len,
                      int64_t layer_idx, int64_t num_hidden_layers, int64_t beta);

/* ---- decode side: one decode step over the compacted cache -------------------------------------------
 * Replaces, per layer and step, the reference's `past_key_value.update` else-branch (llama_model.py:287-289: repeat_kv of
 * the new K/V to H_q heads + torch.cat onto the [1, H_q, cap + t, D] cache) and the SDPA over the result (:306-313).
 * The cache is kept in two parts: the PREFIX [b][H_q][prefix_rows][D] is what kvc_compress wrote (k + W rows per query
 * head; it may live in a buffer with a larger head stride) and is never touched again; the TAIL [b][H_kv][capacity][D]
 * holds the decoded tokens ONCE per KV head.  The call appends the step's `new_rows` K/V rows to the tail in place
 * (rows tail_rows ..) and writes, for every query head and new token i, softmax(q K^T * scaling) V over the head's prefix
 * rows and its KV head's tail rows [0, tail_rows + i + 1) — fp32 accumulation, output in dtype.  All strides in elements;
 * rows are dense (head_dim elements); head_dim 64 or 128; capacity >= tail_rows + new_rows is the caller's business. */
typedef struct kvc_decode_params {
    int32_t dtype;             /* kvc_dtype of every tensor */
    int32_t bsz, n_q_heads, n_kv_heads, head_dim;
    int32_t prefix_rows;       /* rows per query head in the prefix (k + W) */
    int32_t tail_rows;         /* rows already in the tail before this call */
    int32_t new_rows;          /* tokens of this step (rows of q, k_new, v_new) */
    float scaling;             /* softmax scale, 1 / sqrt(head_dim) for Llama / Mistral */
    int32_t reserved;
    int64_t q_stride_b, q_stride_h, q_stride_l;             /* q[b][h_q][i][:] */
    int64_t new_stride_b, new_stride_h, new_stride_l;       /* k_new / v_new [b][h_kv][i][:] */
    int64_t prefix_stride_b, prefix_stride_h;               /* k_prefix / v_prefix [b][h_q][row][:] */
    int64_t tail_stride_b, tail_stride_h;                   /* k_tail / v_tail [b][h_kv][row][:] */
    int64_t out_stride_b, out_stride_h, out_stride_l;       /* out[b][h_q][i][:] */
} kvc_decode_params;

int kvc_decode_step(const kvc_decode_params* p, const void* q, const void* k_new, const void* v_new,
                    const void* k_prefix, const void* v_prefix, void* k_tail, void* v_tail, void* out, void* hip_stream);

/* kvc_decode_step2 (ABI 5): the same step with
 *   - a workspace, so that the rows of one head are shared by several workgroups and merged afterwards (a decode step over a
 *     2 056-row cache reads 1 MB per head: with one workgroup per head 7/8 of the chip idles — 80 us -> see profiles/r03_decode*);
 *     kvc_decode_workspace_bytes(p, ext) says how much; less (or NULL) only reduces the number of splits;
 *   - optionally (ext != NULL) separate strides for v_prefix and ThinK's channel-pruned leading rows
 *     (llama_model_think.py:160-200, cache_utils_think.py:390-424): the first `pruned_rows` rows of a head have their keys in
 *     k_pruned [b][h_q][pruned_rows][pruned_dim] — only the kept channels, in ascending channel order, zero-padded to a multiple of
 *     16 bytes — and are scored against the query's channels chan[b][h_q][0..pruned_dim) (int16, -1 = padding column); their
 *     values are rows [0, pruned_rows) of v_prefix, the full-channel prefix keys k_prefix[0..prefix_rows) pair with
 *     v_prefix rows [pruned_rows, pruned_rows + prefix_rows). */
typedef struct kvc_decode_ext {
    int64_t v_prefix_stride_b, v_prefix_stride_h;           /* v_prefix [b][h_q][row][:]; 0 = the same as prefix_stride_* */
    int32_t pruned_rows, pruned_dim;
    int64_t pruned_stride_b, pruned_stride_h;               /* k_pruned [b][h_q][row][pruned_dim] */
    int64_t chan_stride_b, chan_stride_h;                   /* chan [b][h_q][pruned_dim] (elements of int16) */
} kvc_decode_ext;
size_t kvc_decode_workspace_bytes(const kvc_decode_params* p, const kvc_decode_ext* ext /* nullable */);
int kvc_decode_step2(const kvc_decode_params* p, const kvc_decode_ext* ext /* nullable */, const void* q, const void* k_new, const void* v_new,
                     const void* k_prefix, const void* v_prefix, void* k_tail, void* v_tail,
                     const void* k_pruned /* nullable */, const int16_t* chan /* nullable */, void* out,
                     void* workspace /* nullable */, size_t workspace_bytes, void* hip_stream);

/* kvc_decode_step_rows: kvc_decode_step2 with ext == NULL for a BATCH whose rows hold different numbers of prefix rows (left-padded
 * prompts of unequal length, each compressed as the sequence it is alone).  Batch row b sees prefix rows [0, prefix_rows_b[b]) of
 * every one of its heads and the tail as in kvc_decode_step; nothing at or behind row prefix_rows_b[b] of a prefix buffer is read.
 *   - prefix_rows_b: device array of bsz int32, read by the kernels only (the host never looks at it; it may be the product of
 *     earlier work on the stream).  p->prefix_rows is the number of rows the prefix buffers hold per head: every entry is clamped
 *     to [0, p->prefix_rows] on the device, so no value of the array makes the call read outside the buffers.
 *   - the tail is uniform: tail_rows and new_rows hold for every batch row, and the step's rows are appended as in kvc_decode_step.
 *   - workspace: kvc_decode_rows_workspace_bytes(p) bytes, 16-byte aligned, sized from the bound; less (or NULL) only reduces the
 *     number of splits.  Its contents before the call do not matter: a split that has no rows for a short batch row writes nothing
 *     and is not read.
 * Two kernels for the whole batch (attention, merge of the splits) and one for the append; every argument is checked before any
 * pointer is used; enqueue-only: no allocation, no synchronisation. */
size_t kvc_decode_rows_workspace_bytes(const kvc_decode_params* p);
int kvc_decode_step_rows(const kvc_decode_params* p, const int32_t* prefix_rows_b /* device, [bsz] */,
                         const void* q, const void* k_new, const void* v_new, const void* k_prefix, const void* v_prefix,
                         void* k_tail, void* v_tail, void* out, void* workspace /* nullable */, size_t workspace_bytes, void* hip_stream);

/* kvc_decode_step_dev: kvc_decode_step_rows (kvc_decode_step2 with ext == NULL when prefix_rows_b is NULL) with the TAIL LENGTH read
 * on the device, so that the call can be captured in a HIP graph and replayed while the cache grows.  The tail buffers hold
 * tail_capacity rows per KV head;
 *     T = clamp(*tail_rows_dev, 0, tail_capacity - new_rows)
 * is read by the kernels only, p->tail_rows is ignored.  The step's rows are appended at tail row T; token i of batch row b sees
 * prefix rows [0, P_b) and tail rows [0, T + i + 1), P_b = prefix_rows_b[b] clamped to [0, p->prefix_rows], or p->prefix_rows.
 *   - THE RULE: nothing the host passes depends on T.  The grid and the rows of a split come from the bound
 *     p->prefix_rows + tail_capacity; a workgroup whose first row is at or past the visible rows returns before it loads anything
 *     and writes nothing, and the merge of the splits reads only those that ran.  Two calls with the same arguments differ only in
 *     what the device finds in the counter: a captured call replays correctly for every later length.
 *   - the library only READS the counter; the caller advances it by new_rows, in stream order, after the call (inside a captured
 *     region: a device-side add), and moves to larger tail buffers before T + new_rows would pass tail_capacity.
 *   - the clamp: no counter value makes a kernel read or write outside rows [0, tail_capacity) of the tail buffers.  Tail rows at
 *     or behind T + new_rows are neither read nor written.
 *   - workspace: kvc_decode_dev_workspace_bytes(p, tail_capacity) bytes, 16-byte aligned, sized from the bound; less (or NULL)
 *     only reduces the number of splits.  Its contents before the call do not matter.  A captured call must own its workspace
 *     (and `out`) for as long as the graph lives.
 * Every argument is checked before any pointer is used (tail_capacity < new_rows and a NULL counter are KVC_ERR_INVALID);
 * enqueue-only: no allocation, no synchronisation, no host read, no kernel attribute set on the launch path. */
size_t kvc_decode_dev_workspace_bytes(const kvc_decode_params* p, int32_t tail_capacity);
int kvc_decode_step_dev(const kvc_decode_params* p, int32_t tail_capacity,
                        const int32_t* tail_rows_dev /* device, 1 int32 */,
                        const int32_t* prefix_rows_b /* device [bsz], nullable: NULL = p->prefix_rows for every row */,
                        const void* q, const void* k_new, const void* v_new,
                        const void* k_prefix, const void* v_prefix, void* k_tail, void* v_tail,
                        void* out, void* workspace /* nullable */, size_t workspace_bytes, void* hip_stream);

/* kvc_decode_step_dev_ring: kvc_decode_step_dev that also RECORDS THE STEP'S QUERIES in a ring, so that a later kvc_decode_compress
 * finds the window's queries without a launch of its own.  q_ring [b][H_q][ring_rows][D] (rows dense, ring_stride_b / ring_stride_h in
 * elements), ring_rows = W >= 1.  With T the clamped counter value the step reads (above),
 *     query row i of the step is copied byte for byte to ring slot (T + i) % W, for every i >= new_rows - W;
 * older rows of the step are not recorded, so every slot has at most one writer in a call, and slots the step does not own are not
 * touched.  A kvc_decode_compress with ring_start = T_end % W, T_end the tail rows at that moment (>= W, all appended through this
 * entry), then finds window row w at slot (ring_start + w) % W.  The ring must not overlap any other tensor of the call.
 * Everything else is kvc_decode_step_dev's contract word for word — the clamp, the plan of the bound, the workspace
 * (kvc_decode_dev_workspace_bytes), the checks before any pointer is used, enqueue-only — and the call issues as many kernels: the ring
 * rows are written by the launch that appends K / V.  ring_rows < 1, a NULL or misaligned q_ring, a ring stride that is not a
 * multiple of 16 bytes or is smaller than the ring's extent: KVC_ERR_INVALID. */
int kvc_decode_step_dev_ring(const kvc_decode_params* p, int32_t tail_capacity,
                             const int32_t* tail_rows_dev /* device, 1 int32 */,
                             const int32_t* prefix_rows_b /* device [bsz], nullable */,
                             const void* q, const void* k_new, const void* v_new,
                             const void* k_prefix, const void* v_prefix, void* k_tail, void* v_tail, void* out,
                             void* q_ring, int32_t ring_rows, int64_t ring_stride_b, int64_t ring_stride_h,
                             void* workspace /* nullable */, size_t workspace_bytes, void* hip_stream);

/* ---- decode-stage compression: re-compress the SPLIT decode cache in place (the reference's README TODO "Support KV cache
 * compression at decoding stage") ---------------------------------------------------------------------------------------------
 * The cache of one layer is the prefix [b][H_q][P][D] (per query head) and the tail [b][H_kv][T][D] (per KV head, the decoded
 * rows kvc_decode_step appended).  With G = n_q_heads / n_kv_heads and L = P + T, the call computes EXACTLY what kvc_compress
 * computes (dot_mode EXACT, this tie_mode) for
 *     K[b][h][r] = r < P ? k_prefix[b][h][r] : k_tail[b][h / G][r - P]      (and V alike), r in [0, L), n_kv_heads = H_q,
 *     query rows L-W .. L-1 = the W rows of the query ring, window row w at ring row (ring_start + w) % W,
 *     p->k rows kept besides the W window rows,
 * without materialising K: k_out / v_out [b][H_q][k + W][D] receive cat(K[idx], K[L-W:L]) — the last W rows always come from
 * the tail (T >= W) — idx_out [b][H_q][k] int64 the indices in this virtual row numbering, scores_out [b][H_q][L-W] dtype the
 * pooled scores (both nullable; StreamingLLM: idx = arange(k), idx_out must be NULL, scores_out is not written).
 * Stages: a two-segment window scan (the d-ascending fp32 fmaf chain, the reference's three roundings and the local causal
 * mask), kvc_compress's softmax / pooling stage, its selection, and a two-source gather.  dot_mode mfma16 does not apply here.
 * Limits: those of kvc_compress (head_dim 64 / 128, W <= 64, odd kernel_size <= 63, 0 <= k <= L - W, L > W, tie-mode limits),
 * T >= W, every pointer and stride 16-byte aligned, and k_out / v_out disjoint from each other, the prefix and the tail (the
 * output never aliases the input: a caller alternates two prefix buffers).  Enqueue-only: no allocation, no synchronisation.
 * Workspace: kvc_decode_compress_workspace_bytes(p) bytes, 256-byte aligned (0 for StreamingLLM). */
typedef struct kvc_decode_compress_params {
    int32_t method;                 /* KVC_SNAPKV, KVC_PYRAMIDKV or KVC_STREAMINGLLM */
    int32_t dtype, bsz, n_q_heads, n_kv_heads, head_dim;
    int32_t prefix_rows, tail_rows; /* P (per query head), T >= window (per KV head); L = P + T */
    int32_t window, k, kernel_size, pooling, tie_mode;
    int32_t ring_start;             /* window row w is ring row (ring_start + w) % window */
    int64_t ring_stride_b, ring_stride_h;           /* q ring [b][h_q][window][D], rows dense */
    int64_t prefix_stride_b, prefix_stride_h;       /* k_prefix / v_prefix [b][h_q][row][D] */
    int64_t tail_stride_b, tail_stride_h;           /* k_tail / v_tail [b][h_kv][row][D] */
    int64_t out_stride_b, out_stride_h;             /* k_out / v_out [b][h_q][row][D] */
} kvc_decode_compress_params;
size_t kvc_decode_compress_workspace_bytes(const kvc_decode_compress_params* p);
int kvc_decode_compress(const kvc_decode_compress_params* p, const void* q_ring, const void* k_prefix, const void* v_prefix,
                        const void* k_tail, const void* v_tail, void* k_out, void* v_out, int64_t* idx_out /* nullable */,
                        void* scores_out /* nullable */, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- heavy hitters at decode time (H2O's own rule: evict by the attention every later query paid) ---------------------------------
 * Every stored row of the SPLIT decode cache carries an fp32 SCORE per QUERY head: score_prefix [b][H_q][prefix capacity] for the
 * prefix rows and score_tail [b][H_q][tail capacity] for the tail rows (a tail row's K / V are shared by the G query heads of its
 * KV head, its score is not).
 *
 * kvc_decode_step_scored: kvc_decode_step2 with ext == NULL, and for every new token i of the step, in ascending i, and every row
 * r visible to it (its own row included)
 *     score[h][r] += p_i[h][r],      p_i[h] = the softmax the step's attention uses for token i and head h,
 * in fp32: p = exp2(s - M) / Lsum with s the row's log2-domain logit (the fp32 fmaf chain of the attention kernel), M and Lsum the
 * merged maximum and sum of the (head, token).  A row appended by this step starts from 0: what score_tail rows
 * [tail_rows, tail_rows + new_rows) held before the call does not matter, nor do the contents of the workspace.  Nothing at or
 * behind the visible rows is read or written (K, V, scores).  Every row's probability is owned by one thread: no atomics, the
 * result does not depend on scheduling.  `out` has kvc_decode_step2's bytes (the split plan is that of a kvc_decode_step2 call
 * with its full workspace).  Launches: append, attention, merge of the splits (more than one split only), scoring — one more than
 * kvc_decode_step2.  Workspace: kvc_decode_scored_workspace_bytes(p) bytes, 16-byte aligned, REQUIRED (it holds the logits
 * [b * H_q][new_rows][prefix_rows + tail_rows + new_rows] fp32 besides the splits' partial results).  Score strides in floats,
 * score pointers 4-byte aligned.  Every argument is checked before any pointer is used; enqueue-only. */
typedef struct kvc_decode_scored_params {
    kvc_decode_params step;                                 /* as for kvc_decode_step2 */
    int64_t score_prefix_stride_b, score_prefix_stride_h;   /* score_prefix [b][h_q][row], >= prefix_rows per head */
    int64_t score_tail_stride_b, score_tail_stride_h;       /* score_tail [b][h_q][row], >= tail_rows + new_rows per head */
} kvc_decode_scored_params;
size_t kvc_decode_scored_workspace_bytes(const kvc_decode_scored_params* p);
int kvc_decode_step_scored(const kvc_decode_scored_params* p, const void* q, const void* k_new, const void* v_new,
                           const void* k_prefix, const void* v_prefix, void* k_tail, void* v_tail,
                           float* score_prefix, float* score_tail, void* out,
                           void* workspace, size_t workspace_bytes, void* hip_stream);

/* kvc_decode_step_dev_scored: kvc_decode_step_scored with the LENGTHS read on the device, so that H2O's scored step can be captured in
 * a HIP graph and replayed while the cache grows and is evicted.  The contract is kvc_decode_step_dev's word for word plus
 * kvc_decode_step_scored's score rule.  The tail buffers hold tail_capacity rows per KV head, score_tail tail_capacity scores per
 * query head;
 *     T = clamp(*tail_rows_dev, 0, tail_capacity - new_rows)
 * is read by the kernels only, p->step.tail_rows is ignored.  P_b = prefix_rows_b[b] clamped to [0, p->step.prefix_rows], or
 * p->step.prefix_rows when the pointer is NULL.  The step's rows are appended at tail row T; token i of batch row b sees prefix rows
 * [0, P_b) and tail rows [0, T + i + 1); virtual row r is prefix row r for r < P_b, else tail row r - P_b.
 *   - THE RULE: nothing the host passes depends on T (or on P_b).  The grids, the rows of a split and the row stride of the logits
 *     come from the bound p->step.prefix_rows + tail_capacity (kvc_decode_step_dev's plan with its full workspace); a workgroup
 *     whose first row is at or past the visible rows returns before it loads anything and writes nothing, and the merge of the
 *     splits and the scoring read only the splits that ran.  The library only READS the counter and the prefix lengths.
 *   - scores: for every new token i in ascending order and every virtual row r visible to it (its own row included)
 *     score[h][r] += exp2(s - M) / Lsum in fp32, s the row's log2-domain logit from the attention kernel's fmaf chain, (M, Lsum) of
 *     the (head, token) merged over the splits that ran, in the order of the merge of the splits.  Prefix rows use score_prefix
 *     [b][H_q][>= prefix_rows], tail rows score_tail [b][H_q][>= tail_capacity], one score per query head.  A row appended by this
 *     step starts from 0, whatever its slot held.
 *   - never touched: prefix score slots [P_b, prefix_rows) and tail score slots at or past T + new_rows are neither read nor written;
 *     the same holds for K, V and the workspace behind the visible rows.  No atomics: every probability is owned by one thread, the
 *     result does not depend on scheduling.  No counter value makes a kernel read or write outside the buffers.
 *   - `out` has kvc_decode_step_dev's bytes for the same arguments and its full workspace; when T + new_rows == tail_capacity and
 *     every P_b == prefix_rows (so that the two split plans coincide), `out` and every score are kvc_decode_step_scored's bit for bit.
 *   - workspace: kvc_decode_dev_scored_workspace_bytes(p, tail_capacity) bytes, 16-byte aligned, REQUIRED in full (NULL, misaligned
 *     or short: KVC_ERR_WORKSPACE): the partial results of every split of the bound's plan — (M, Lsum) are stored with one split
 *     too — and the logits [b * H_q][new_rows][prefix_rows + tail_capacity] fp32, indexed by virtual row.  Its contents before the
 *     call do not matter.  A captured call must own its workspace (and `out`) for as long as the graph lives.
 *   - launches: append, attention, merge of the splits (only when the plan has several), scoring — at most one more than
 *     kvc_decode_step_dev.
 * Every argument is checked before any pointer is used: everything kvc_decode_step_dev checks, then NULL score pointers
 * (KVC_ERR_INVALID; score_prefix may be NULL when prefix_rows == 0), score pointers that are not 4-byte aligned (KVC_ERR_ALIGNMENT),
 * score strides (in floats) smaller than prefix_rows / tail_capacity, and score buffers that overlap each other or `out`
 * (KVC_ERR_INVALID).  Enqueue-only: no allocation, no synchronisation, no host read, no kernel attribute set on the launch path. */
size_t kvc_decode_dev_scored_workspace_bytes(const kvc_decode_scored_params* p, int32_t tail_capacity);
int kvc_decode_step_dev_scored(const kvc_decode_scored_params* p, int32_t tail_capacity,
                               const int32_t* tail_rows_dev /* device, 1 int32 */,
                               const int32_t* prefix_rows_b /* device [bsz], nullable: NULL = prefix_rows for every row */,
                               const void* q, const void* k_new, const void* v_new,
                               const void* k_prefix, const void* v_prefix, void* k_tail, void* v_tail,
                               float* score_prefix, float* score_tail, void* out,
                               void* workspace, size_t workspace_bytes, void* hip_stream);

/* kvc_decode_evict: the S = P + T rows of one layer become k + W rows.  With the virtual row numbering of kvc_decode_compress
 * (row r < P: prefix row r of query head h; else tail row r - P of KV head h / G) and score[h][r] read from score_prefix /
 * score_tail alike:
 *     idx[h] = topk(score[h][0 : S - W], k).indices     tie_mode as kvc_select defines it for fp32 scores, no pooling
 *     k_out[h] = cat(K[h][idx[h]], K[h][S - W : S]),  v_out alike,  score_out[h] = cat(score[h][idx[h]], score[h][S - W : S])
 * — every kept row keeps its score.  Stages: the candidates' scores laid out as one fp32 row per head, kvc_select's kernels, one
 * gather launch for K, V and the scores.  k_out / v_out [b][H_q][k + W][D], score_out [b][H_q][k + W] fp32, idx_out (nullable)
 * [b][H_q][k] int64.  Limits: head_dim 64 / 128, T >= W >= 1, 0 <= k <= S - W, kvc_select's tie-mode limits; every K / V pointer
 * and stride 16-byte aligned, score pointers 4-byte aligned; k_out / v_out disjoint from each other, the prefix and the tail,
 * score_out from score_prefix and score_tail (the output never aliases the input: a caller alternates two prefix buffers, each
 * with its score buffer).  Workspace: kvc_decode_evict_workspace_bytes(p) bytes, 256-byte aligned.  Enqueue-only. */
typedef struct kvc_decode_evict_params {
    int32_t dtype, bsz, n_q_heads, n_kv_heads, head_dim;
    int32_t prefix_rows, tail_rows; /* P (per query head), T >= window (per KV head); S = P + T */
    int32_t window, k, tie_mode;
    int64_t prefix_stride_b, prefix_stride_h;               /* k_prefix / v_prefix [b][h_q][row][D] */
    int64_t tail_stride_b, tail_stride_h;                   /* k_tail / v_tail [b][h_kv][row][D] */
    int64_t out_stride_b, out_stride_h;                     /* k_out / v_out [b][h_q][row][D] */
    int64_t score_prefix_stride_b, score_prefix_stride_h;   /* floats */
    int64_t score_tail_stride_b, score_tail_stride_h;
    int64_t score_out_stride_b, score_out_stride_h;
} kvc_decode_evict_params;
size_t kvc_decode_evict_workspace_bytes(const kvc_decode_evict_params* p);
int kvc_decode_evict(const kvc_decode_evict_params* p, const void* k_prefix, const void* v_prefix, const void* k_tail,
                     const void* v_tail, const float* score_prefix, const float* score_tail, void* k_out, void* v_out,
                     float* score_out, int64_t* idx_out /* nullable */, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- quantized decode cache (KIVI-style, --quant_method kivi --nbits N of the reference's run scripts) ----------------------
 * Rule: asymmetric round-to-nearest, every group on its own in fp32 with the inputs widened exactly.  KEYS are grouped per
 * channel (G = group_size consecutive stored rows share one (scale, zero) per channel; a segment whose rows are not a multiple
 * of G ends with a partial group that gets its own min / max); VALUES are grouped per token (G consecutive channels of one row
 * share one (scale, zero)).  With qmax = 2^nbits - 1 and mn, mx the group's minimum and maximum:
 *     scale = (mx - mn) / qmax                                          fp32, correctly rounded division
 *     code  = scale > 0 ? clamp(rint((x - mn) / scale), 0, qmax) : 0     rint = round half to even
 *     x'    = fmaf(code, scale, mn)                                      the de-quantized value
 * (the library is built with -ffp-contract=off and correctly rounded fp32 division, so codes, scales and zeros are
 * reproducible bit for bit by any fp32 restatement).  Inputs are assumed finite: a NaN or an infinity in a group gives
 * unspecified codes for that group.  nbits 2, 4 or 8; G 32, 64 or 128 dividing head_dim; head_dim 64 or 128; bf16 / fp16 / fp32.
 *
 * Layout of one segment of `capacity` rows per head (b, h) — the same for the prompt, the quantized tail, keys and values:
 *   codes  [b][h][capacity][head_dim * nbits / 8] bytes, rows dense: channel d of a row sits at bit d * nbits of the row,
 *          little-endian within each byte (channel 0 in the low bits of byte 0);
 *   key metadata   [b][h][ceil(capacity / G)][2][head_dim] fp32: per group the scale of every channel, then the zero (= mn)
 *                  of every channel;
 *   value metadata [b][h][capacity][head_dim / G][2] fp32: per row and channel group the pair (scale, zero).
 * Code strides are in bytes (multiples of 16), metadata strides in floats (key: multiples of 4, value: of 2), source /
 * destination strides in elements. */
typedef enum kvc_quant_mode { KVC_QUANT_KEYS = 0, KVC_QUANT_VALUES = 1 } kvc_quant_mode;

typedef struct kvc_quant_params {      /* kvc_quantize_rows / kvc_dequantize_rows: rows [row0, row0 + rows) of one segment */
    int32_t dtype, bsz, n_heads, head_dim;
    int32_t nbits, group_size;
    int32_t mode;                      /* kvc_quant_mode */
    int32_t row0;                      /* first segment row written / read (keys: a multiple of group_size) */
    int32_t rows;                      /* rows quantized / de-quantized (0: nothing to do) */
    int32_t capacity;                  /* rows per head the code and metadata buffers hold */
    int64_t src_stride_b, src_stride_h, src_stride_l;       /* elements: the [b][h][row][d] source (quantize) or destination */
    int64_t code_stride_b, code_stride_h;                   /* bytes */
    int64_t meta_stride_b, meta_stride_h;                   /* floats */
} kvc_quant_params;

/* quantize: src rows [0, rows) -> segment rows [row0, row0 + rows) (codes and this mode's metadata; key groups start at row0).
 * dequantize: segment rows [row0, row0 + rows) -> dst rows [0, rows) in dtype (x' rounded to dtype). */
int kvc_quantize_rows(const kvc_quant_params* p, const void* src, uint8_t* codes, float* meta, void* hip_stream);
int kvc_dequantize_rows(const kvc_quant_params* p, const uint8_t* codes, const float* meta, void* dst, void* hip_stream);

typedef struct kvc_quant_seg {         /* one quantized segment of the decode cache (layout above) */
    const uint8_t* k_codes; const uint8_t* v_codes;
    const float* k_meta; const float* v_meta;
    int32_t rows, capacity;            /* rows in use / rows per head the buffers hold */
    int64_t code_stride_b, code_stride_h;                   /* bytes, k_codes and v_codes alike */
    int64_t k_meta_stride_b, k_meta_stride_h, v_meta_stride_b, v_meta_stride_h;     /* floats */
} kvc_quant_seg;

/* kvc_decode_step_quant: kvc_decode_step2 over a quantized cache of four segments, one attention per (query head, new token):
 *   prefix [b][H_q]   the compressed prompt quantized once (rows = k + W);
 *   qtail  [b][H_kv]  decoded rows quantized in whole key groups, append-only (rows a multiple of G);
 *   residual k_res / v_res [b][H_kv][res_capacity][head_dim] in dtype: res_rows full-precision rows;
 *   the step's new_rows K / V rows, which the call appends to the residual at row res_rows (as kvc_decode_step does to its tail).
 * Token i sees the prefix, the quantized tail and residual rows [0, res_rows + i + 1).  The attention runs over the
 * de-quantized values x' (above) with fp32 accumulation; output [b][h_q][i][:] in dtype.  Moving residual rows onto the
 * quantized tail (kvc_quantize_rows) is the caller's business: res_rows < residual_length on entry, residual_length a positive
 * multiple of G.  Workspace: kvc_decode_quant_workspace_bytes(p) (less, or NULL, only reduces the number of splits). */
typedef struct kvc_decode_quant_params {
    int32_t dtype, bsz, n_q_heads, n_kv_heads, head_dim;
    int32_t nbits, group_size, residual_length;
    int32_t res_rows, res_capacity, new_rows;
    float scaling;
    int64_t q_stride_b, q_stride_h, q_stride_l;             /* q[b][h_q][i][:] */
    int64_t new_stride_b, new_stride_h, new_stride_l;       /* k_new / v_new [b][h_kv][i][:] */
    int64_t res_stride_b, res_stride_h;                     /* k_res / v_res [b][h_kv][row][:], rows dense */
    int64_t out_stride_b, out_stride_h, out_stride_l;       /* out[b][h_q][i][:] */
} kvc_decode_quant_params;
size_t kvc_decode_quant_workspace_bytes(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix, const kvc_quant_seg* qtail);
int kvc_decode_step_quant(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix, const kvc_quant_seg* qtail,
                          const void* q, const void* k_new, const void* v_new, void* k_res, void* v_res, void* out,
                          void* workspace /* nullable */, size_t workspace_bytes, void* hip_stream);

/* kvc_decode_step_quant_dev: kvc_decode_step_quant with BOTH GROWING LENGTHS read on the device, in the spirit of kvc_decode_step_dev,
 * so that the quantized step can be captured in a HIP graph and replayed while rows are decoded and moved onto the quantized tail.
 *   prefix    prefix->rows stays a host constant (the prompt is quantized once);
 *   qtail     the buffers hold qtail->capacity rows (a multiple of group_size), qtail->rows is ignored:
 *                 Tq = clamp(*qtail_rows_dev, 0, qtail->capacity)
 *   residual  the buffers hold p->res_capacity rows, p->res_rows is ignored:
 *                 Rr = clamp(*res_rows_dev, 0, p->res_capacity - new_rows)
 * Both words are read by the kernels only.  The step's rows are appended at residual row Rr; token i sees prefix rows [0, P), quantized
 * tail rows [0, Tq) and residual rows [0, Rr + i + 1), in this virtual row order.
 *   - THE RULE: nothing the host passes depends on Tq or Rr.  The grid and the rows of a split (a multiple of 64) come from the bound
 *     P + qtail->capacity + res_capacity — the plan kvc_decode_step_quant makes for that many rows; a workgroup whose first virtual
 *     row is at or past the visible rows returns before it loads anything and writes nothing, and the merge of the splits counts the
 *     splits that ran and reads only those.  A captured call replays correctly for every later pair of lengths.
 *   - the library only READS the two words; the caller advances the residual word by new_rows in stream order after the call (inside
 *     a captured region: a device-side add) and, when it moves residual rows onto the tail (kvc_quantize_rows at row0 = Tq, between
 *     two replays), adds their number to the tail word and takes it off the residual word.
 *   - the clamps: no value of either word makes a kernel read or write outside the buffers.  Codes, metadata and residual rows behind
 *     the visible rows are neither read nor written (key metadata is read per group of a visible row).
 *   - arithmetic: kvc_decode_step_quant's.  When Tq == qtail->capacity and Rr + new_rows == res_capacity the two plans coincide and
 *     `out` and the appended residual rows are kvc_decode_step_quant's bit for bit.
 *   - workspace: kvc_decode_quant_dev_workspace_bytes(p, prefix, qtail) bytes, 16-byte aligned, sized from the bound; less (or NULL)
 *     only reduces the number of splits.  Its contents before the call do not matter.  A captured call must own its workspace (and
 *     `out`) for as long as the graph lives.
 * No outliers (the KVQuant form keeps host-read pool counters).  Every argument is checked before any pointer is used: everything
 * kvc_decode_step_quant checks (with the two ignored lengths taken as 0), a NULL word, res_capacity < new_rows and a qtail->capacity
 * that is not a multiple of group_size (KVC_ERR_INVALID).  Enqueue-only: no allocation, no synchronisation, no host read, no kernel
 * attribute set on the launch path. */
size_t kvc_decode_quant_dev_workspace_bytes(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix, const kvc_quant_seg* qtail);
int kvc_decode_step_quant_dev(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix, const kvc_quant_seg* qtail,
                              const int32_t* qtail_rows_dev /* device, 1 int32 */, const int32_t* res_rows_dev /* device, 1 int32 */,
                              const void* q, const void* k_new, const void* v_new, void* k_res, void* v_res, void* out,
                              void* workspace /* nullable */, size_t workspace_bytes, void* hip_stream);

/* ---- quantized cache with exact outliers (KVQuant-style "dense-and-sparse", --quant_method kvquant) ------------------------
 * Split: T' = threshold rounded to dtype (round to nearest even; fp32 uses it as is).  Element x is an OUTLIER iff x < -T' or
 * x > T' (so +-inf are outliers and NaN is not).  The DENSE input is x with every outlier replaced by +0; its codes and metadata
 * follow the rule above unchanged (the zeros take part in their group's min / max).  De-quantized value: x'' = x at an outlier,
 * otherwise x' = fmaf(code, scale, mn).  Groups holding +-inf are therefore well defined; groups with NaN stay unspecified.
 *
 * Sparse layout, one POOL per (segment, keys or values), indexed by the batch row like every other buffer:
 *   chan    [b][pool_capacity] uint8     channel of the entry
 *   val     [b][pool_capacity] dtype     its exact value
 *   used    [b] int32                    entries handed out so far (device counter)
 *   rowinfo [b][h][capacity] uint32      per segment row: (first entry << 8) | count; 0 = no entries
 * A quantize call lays its entries out in (h, row, channel) order starting at used[b] and advances used[b] by the number of
 * outliers it found.  A row whose entries do not all fit below pool_capacity gets rowinfo 0 and no entry is written for it (no
 * byte at or past pool_capacity is ever written); used[b] still advances by the full count, so used[b] > pool_capacity tells the
 * caller that the call overflowed and must be repeated into a larger pool (rows that fit are complete).  pool_capacity < 2^24.
 * All four entry points below are enqueue-only (no allocation, no copy to the host, no synchronisation). */
typedef struct kvc_quant_outliers {
    uint8_t* chan; void* val; int32_t* used; uint32_t* rowinfo;
    int32_t pool_capacity, reserved;
    int64_t pool_stride_b;                                  /* entries between batch rows of chan / val (>= pool_capacity) */
    int64_t rowinfo_stride_b, rowinfo_stride_h;             /* words (rowinfo_stride_h >= the segment's capacity) */
} kvc_quant_outliers;

/* As kvc_quantize_rows, with the split: dense codes / metadata, plus the outliers of rows [row0, row0 + rows) into `outl`
 * (rowinfo of those rows, entries from used[b]).  threshold: finite and > 0. */
int kvc_quantize_rows_outliers(const kvc_quant_params* p, float threshold, const void* src, uint8_t* codes, float* meta,
                               const kvc_quant_outliers* outl, void* hip_stream);
/* As kvc_dequantize_rows, then the outliers of those rows written back exactly. */
int kvc_dequantize_rows_outliers(const kvc_quant_params* p, const uint8_t* codes, const float* meta, const kvc_quant_outliers* outl,
                                 void* dst, void* hip_stream);
/* kvc_decode_step_quant over segments with outliers: prefix_outl / qtail_outl point at TWO descriptors each (keys, then values;
 * rowinfo per query head for the prefix, per KV head for the tail).  A segment without rows needs none (NULL allowed). */
size_t kvc_decode_quant_outliers_workspace_bytes(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix, const kvc_quant_seg* qtail,
                                                 const kvc_quant_outliers* prefix_outl, const kvc_quant_outliers* qtail_outl);
int kvc_decode_step_quant_outliers(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix, const kvc_quant_seg* qtail,
                                   const kvc_quant_outliers* prefix_outl, const kvc_quant_outliers* qtail_outl,
                                   const void* q, const void* k_new, const void* v_new, void* k_res, void* v_res, void* out,
                                   void* workspace /* nullable */, size_t workspace_bytes, void* hip_stream);

/* ---- AdaKV / HeadKV: per-head budgets, ragged ("flattened") cache -----------------------------------
 * Replaces AdaKVCluster.update_kv (pyramidkv_utils.py:674-757), HeadKVCluster.update_kv (:813-878) and, at decode, the
 * repo's native update_flatten_view (csrc/csrc/cuda_api.cu:12-85) + flash_attn_varlen_func (llama_model.py:2363-2390).
 * p->method = KVC_ADAKV or KVC_HEADKV, p->k = base capacity (max_capacity_prompt - window), tie order of the per-head sort
 * exactly torch-CPU's (libstdc++ std::sort).  Three calls, all enqueue-only:
 *   kvc_ragged_plan     scores (window mean + pooling, :647-672) into the workspace; AdaKV: caps_out[b][h] = rows head h keeps
 *                       (device int32; flags_out[b][0] = 1 if values equal to the global threshold span several heads and
 *                       had to be shared out in flattened order — the one place where torch's partial_sort tie order is not
 *                       reproduced).  HeadKV: scores only (the caller owns the capacities).
 *   — the host reads the capacities (the reference's own metadata are host integers, :721-741) and lays out the flat cache:
 *     seg_off[b*H + h] = first row of head h, any spare rows behind a head are for in-place decode appends —
 *   kvc_ragged_compact  per head the first caps[h] indices of its descending sort + the W window rows, K and V, into
 *                       k_flat / v_flat at seg_off[h]; idx_out (nullable) receives the kept indices [b*H][idx_stride].
 *   kvc_ragged_decode_step  appends the step's K/V rows behind every head's segment (once per QUERY head, like the
 *                       reference's flattened cache) and attends over the segment: rows [0, seg_len[h] + appended + i + 1).
 * Workspace: kvc_ragged_workspace_bytes(p) for plan + compact (the same buffer, same stream). */
size_t kvc_ragged_workspace_bytes(const kvc_params* p);
int kvc_ragged_plan(const kvc_params* p, const void* q, const void* k, float floor_ratio, int normalize,
                    int32_t* caps_out, int32_t* flags_out, void* scores_out, void* workspace, size_t workspace_bytes, void* hip_stream);
int kvc_ragged_compact(const kvc_params* p, const void* k, const void* v, const int32_t* caps, const int64_t* seg_off, int rows_max,
                       void* k_flat, void* v_flat, int64_t* idx_out, int64_t idx_stride,
                       void* workspace, size_t workspace_bytes, void* hip_stream);
typedef struct kvc_ragged_decode_params {
    int32_t dtype, bsz, n_q_heads, n_kv_heads, head_dim;
    int32_t appended;          /* rows appended to every segment since the prefill (before this call) */
    int32_t new_rows;          /* tokens of this step */
    float scaling;
    int64_t q_stride_b, q_stride_h, q_stride_l;             /* q[b][h_q][i][:] */
    int64_t new_stride_b, new_stride_h, new_stride_l;       /* k_new / v_new [b][h_kv][i][:] */
    int64_t out_stride_b, out_stride_h, out_stride_l;       /* out[b][h_q][i][:] */
    int32_t slack_rows;        /* ABI 5: spare rows behind every segment (0 = not checked): appended + new_rows beyond it is refused */
    int32_t reserved;
} kvc_ragged_decode_params;
int kvc_ragged_decode_step(const kvc_ragged_decode_params* p, const void* q, const void* k_new, const void* v_new,
                           void* k_flat, void* v_flat, const int64_t* seg_off, const int32_t* seg_len, void* out, void* hip_stream);

/* ---- CAMKVCluster.update_kv (pyramidkv_utils.py:431-513), split at its random draw (ABI 5) --------------
 * The reference scores like SnapKV without pooling (:461-476), then walks the tokens s = start_budget .. q_len - window - 1 in
 * a Python loop (:487-502): merge_prob = colmean[s] / max(max(colmean[:start_budget]), max(colmean[s : s + window])) per head
 * (colmean = torch.mean of the window rows' probabilities), NaN -> 0, inf -> 1, clamped to [0, 1];
 * merge_mask = torch.bernoulli(merge_prob); value[s + 1 .. s + window] += value[s] * merge_mask / window, in place, in dtype
 * arithmetic; finally top-k on the window sums and gather of the keys and of the MERGED values.  colmean does not depend on
 * the merged values, so:
 *   kvc_cam_plan   p->method = KVC_SNAPKV, p->pooling = KVC_POOL_NONE: scores_out [bsz*H_q][q_len - window] (the top-k input)
 *                  and prob_out [bsz*H_q][q_len - window - start_budget] (dtype; token s at column s - start_budget);
 *   (caller)       draws merge_mask = bernoulli(prob) — torch's CPU generator stream in the reference; any draw here;
 *   kvc_cam_merge  v [bsz][H_q][q_len][head_dim] (strides p->v_stride_*, one copy per QUERY head: the masks differ per head),
 *                  updated in place exactly as the loop does given merge_mask (uint8, same shape as prob_out);
 *   kvc_select + kvc_gather (keys from k, values from the merged v) finish the job.
 * start_budget = ceil(start_budget_ratio * q_len) (:479). */
size_t kvc_cam_workspace_bytes(const kvc_params* p);
int kvc_cam_plan(const kvc_params* p, const void* q, const void* k, int start_budget, void* scores_out, void* prob_out,
                 void* workspace, size_t workspace_bytes, void* hip_stream);
int kvc_cam_merge(const kvc_params* p, void* v, const uint8_t* merge_mask, int start_budget, void* hip_stream);

/* ---- L2NormCluster.update_kv (pyramidkv_utils.py:394-429) ------------------------------------------
 * The k = max_capacity_prompt keys of every head with the SMALLEST L2 norm, in ascending norm order, and their values:
 *   token_norms = torch.norm(key_states, p=2, dim=-1)  (:419)  -> argsort ascending (:420) -> gather, first k rows (:423-427).
 * p->method = KVC_L2NORM; p->k = rows kept (1 <= k <= q_len); window, kernel_size, pooling, tie_mode, dot_mode and the q
 * strides are ignored (the reference's cluster takes neither a query nor a window).  The caller decides pass-through
 * (q_len < max_capacity_prompt, or layer_idx in skip_layers: :413-416) and does not call.
 * Norm arithmetic = torch-CPU's (8 fp32 accumulators by d % 8, added 0..7, fp32 sqrt, one rounding to the dtype);
 * order of equal norms = torch-CPU's sort (libstdc++ std::sort on (value, index), ascending).
 * k, v: [b][n_kv_heads][L][D] by the k_/v_ strides; k_out, v_out: [b][n_q_heads][k][D] (p->out_stride_h elements between
 * heads, 0 = dense) — query heads of one KV group receive identical rows, as the reference's expanded tensors do.
 * idx_out [b*n_q_heads][k] int64 and norms_out [b][n_q_heads][L] dtype may be NULL.
 * Workspace: kvc_l2norm_workspace_bytes(p), 256-byte aligned. */
size_t kvc_l2norm_workspace_bytes(const kvc_params* p);
int kvc_l2norm_compress(const kvc_params* p, const void* k, const void* v, void* k_out, void* v_out, int64_t* idx_out,
                        void* norms_out, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- merge_kv(key_states, value_states, indices, window_size, "pivot") (pyramidkv_utils.py:119-170) ------
 * What SnapKV / PyramidKV / H2O update_kv return instead of the plain gather when their cluster was built with merge="pivot"
 * (:337-339): every token selected by NO head ("dropped", the window included) is averaged into the kept key it is most
 * similar to (cosine, first maximum) and its value into the value row of the same number; kept rows become the mean of
 * themselves and what was merged into them.  idx: [b*n_q_heads][p->k] int64 on the device — the indices of the method's
 * top-k (kvc_select / kvc_compress idx_out).  Outputs [b][n_q_heads][k + window][D]: k_out in the reference's key order
 * [window rows, selected rows], v_out in its value order [selected rows, window rows] (the reference's two cats differ, :145 / :147,
 * and the pivot found on the key order is applied to both).  head_dim must be 128 (hard-coded in the reference, :149);
 * 16-bit dtypes.  bsz > 1: the union of selections is taken per batch row (the reference flattens its isin over the batch
 * too, :131-134, and is only ever run with bsz = 1, README.md:29).  pivot_out ([b*n_q_heads][q_len] int32: row [0, drop_len) = pivot of every dropped token, ascending position)
 * and drop_len_out ([b] int32) may be NULL.  Arithmetic: see csrc/kvc_merge.hip.  Workspace: kvc_merge_workspace_bytes(p). */
size_t kvc_merge_workspace_bytes(const kvc_params* p);
int kvc_merge_pivot(const kvc_params* p, const void* k, const void* v, const int64_t* idx, void* k_out, void* v_out,
                    int32_t* pivot_out, int32_t* drop_len_out, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- ThinK channel pruning, key_pruner_query_driven (pyramidkv_utils.py:13-26) ---------------------------
 * What SnapKVCluster.update_think (:349-392) does after its compression: per head the n_prune = int(head_dim * ratio) channels
 * with the smallest mean(q^2 over the last 32 query rows) * mean(k'^2 over the compressed keys) are removed from the compressed
 * keys except the last `recent` rows.  kc: the compressed keys [b*n_heads][rows][head_dim] (rows dense, kc_stride_h elements
 * between heads — kvc_compress's k_out with its out_stride_h); q: the prompt's queries, rows q_len-32 .. q_len-1 are read.
 * Outputs: pruned [b*n_heads][rows - recent][head_dim - n_prune] (kept channels in order), keep [b*n_heads][head_dim] bytes
 * (1 = kept: the reference's returned ~mask), channel_scores [b*n_heads][head_dim] dtype or NULL.  The recent rows stay where
 * they are (kc rows rows-recent ..).  head_dim 64 or 128, q_len >= 32.  Same arithmetic and tie order as torch-CPU
 * (csrc/kvc_think.hip).  No workspace. */
typedef struct kvc_think_params {
    int32_t dtype, bsz, n_heads, q_len, head_dim;
    int32_t rows, recent, n_prune;
    int64_t q_stride_b, q_stride_h, q_stride_l;     /* elements */
    int64_t kc_stride_h;                            /* elements between heads of kc (>= rows * head_dim) */
} kvc_think_params;
int kvc_think_prune(const kvc_think_params* p, const void* q, const void* kc, void* pruned, uint8_t* keep, void* channel_scores,
                    void* hip_stream);

/* Debug/parity aid: byte offsets inside the workspace of the intermediates kvc_scores leaves behind.
 * offs[0]=logits [b][h][L][W] dtype, offs[1]=row max [b][h][W] f32, offs[2]=row sum [b][h][W] f32.
 * Returns KVC_OK or an error. */
int kvc_workspace_layout(const kvc_params* p, size_t offs[3]);

#ifdef __cplusplus
}
#endif
#endif /* KVC_H_ */
