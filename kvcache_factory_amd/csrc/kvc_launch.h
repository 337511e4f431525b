// kvc_launch.h — argument blocks and host launch functions shared by the kernel files and kvc_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kvc {

// One launch of every kernel can serve up to KVC_MAX_ITEMS independent "items" (the layers of one prompt:
// kvc_compress_batch) — same shapes, per-item tensors and per-item k.  Pointer tables travel in the kernel arguments
// (no device-side copies); blockIdx.z (or .y for the per-head kernels) is the item.  kvc_compress is the 1-item case.
constexpr int KVC_MAX_ITEMS = 32;
struct PtrTable { const void* p[KVC_MAX_ITEMS]; };
struct IntTable { int v[KVC_MAX_ITEMS]; };
struct I64Table { int64_t v[KVC_MAX_ITEMS]; };

struct ScoreView {         // one item's pointers, resolved at kernel entry
    const void* q; const void* k;
    void* logits; float* pmax; float* rowmax; float* rowsum; void* scores;
    float* part16;         // [bsz*Hq][W/16][n_pad] fp32: in-order sums of 16 window rows (softmax_rows16_kernel), or null
};

struct ScoreArgs {
    PtrTable q, k, scores; // per item; scores [bsz*Hq][L-W] dtype
    char* ws;              // workspace of item 0; item i lives ws_item_stride bytes further
    int64_t ws_item_stride;
    // byte offsets inside an item's workspace:
    int64_t off_logits;    // [bsz*Hq][L][W] dtype
    int64_t off_pmax;      // [bsz*Hq][n_tiles][W] fp32
    int64_t off_rowmax;    // [bsz*Hq][W] fp32
    int64_t off_rowsum;    // [bsz*Hq][W] fp32
    int64_t off_part16;    // [bsz*Hq][W/16][n_pad] fp32, or -1 (window not a multiple of 16, fp32)
    int n_items;
    int64_t q_stride_b, q_stride_h, q_stride_l;
    int64_t k_stride_b, k_stride_h, k_stride_l;
    int bsz, n_q_heads, n_kv_heads, group, q_len, window;
    int n_tiles, kernel_size, pooling;
    int fast_dot;          // 1: packed bf16/fp16 MFMA scan (tolerance mode), 0: exact f32 fmaf-chain MFMA
    int window_mean;       // 1: the window rows are averaged (AdaKV / HeadKV, .mean(dim=-2)) instead of summed
    int stage_mask;        // bits 0-2: 0 = all, else bit0 logits, bit1 rowsum, bit2 pool (profiling aid); bit3 / bit4: force the split / fused softmax path
    float sqrt_d;
    unsigned long long* dbg;   // diagnostic stamps (KVC_STAMPS builds only), else null
};

struct H2OArgs {
    const void* q; const void* k;
    void* S;               // [bsz*Hq][s_rows][L] dtype logits of the query rows [row0, row0 + rows) (exact mode)
    int row0, rows, s_rows;    // the chunk of query rows in flight and the row capacity of S per head (launcher-set)
    int fast;              // 1: dot_mode mfma16 — two recomputing passes on the bf16/fp16 MFMA, no S at all
    void* kt;              // exact mode, fused form: [bsz*Hkv][ceil(L/16)][D/32][64 lanes][16 B], K as the MFMA B operand is loaded
    int legacy;            // 1: round 2's materialising exact kernels (debug_stage_mask bit 11)
    float* rowmax;         // [bsz*Hq][L]   (fast mode: -max * log2(e))
    float* rinv;           // [bsz*Hq][L]
    float* part;           // [bsz*Hq][n_blk + 1][n_pad] column sums of each 256-row block (+ the leftover rows), or null
    void* scores;          // [bsz*Hq][L-W] dtype
    int64_t q_stride_b, q_stride_h, q_stride_l;
    int64_t k_stride_b, k_stride_h, k_stride_l;
    int bsz, n_q_heads, n_kv_heads, group, q_len, window;
    float sqrt_d;
};

struct GatherArgs {
    PtrTable src, out, idx;                           // per item; idx entry may be null (identity)
    IntTable k;                                       // per item
    int64_t stride_b, stride_h, stride_l;             // elements
    I64Table out_head_bytes;                          // per item: bytes between heads of `out`; 0 = dense ((k + window) rows)
    int bsz, n_q_heads, group, q_len, window, k_max, row_bytes, esize, n_items;
};

struct SelectArgs {
    PtrTable scores;       // per item: [bsz*Hq][n] dtype
    PtrTable idx;          // per item: int64 [bsz*Hq][k_item]
    IntTable k;            // per item
    int n, k_max, heads;   // heads = bsz*Hq
    int n_items;
    int pow2;              // next power of two >= k_max
    int fuse;              // 1: also gather K (gk) and V (gv) rows of the head in the same workgroup
    int members_only;      // exact mode, large partial_sort heaps: the caller needs the selected SET only (AdaKV's per-head counts)
    GatherArgs gk, gv;
};

struct GatherPair { GatherArgs t[2]; int count; };    // K and V compacted by one launch

struct RaggedSortArgs {    // sort_prefix_kernel (AdaKV / HeadKV)
    const void* scores;    // [heads][n] dtype
    const int32_t* caps;   // [heads] device: how many leading indices of the descending sort each head keeps
    int64_t* idx_out;      // [heads][out_stride]
    int n, heads, out_stride;
    int want_fixed = 0;    // caps == nullptr: leading indices kept by every head (0 = the whole sort)
    int ascending = 0;     // 1: torch-CPU's ascending sort (L2Norm's argsort, pyramidkv_utils.py:420)
};

struct MergeArgs {         // merge_kv pivot merge (kvc_merge.hip)
    const void* k; const void* v;
    const int64_t* idx;    // [bsz * n_q_heads][n_keep]: the select stage's indices
    void* k_out; void* v_out;
    int32_t* mask;         // [bsz][q_len] workspace
    int32_t* drop;         // [bsz][q_len]
    int32_t* drop_len;     // [bsz]
    float* kn;             // [bsz * n_q_heads][rows][128] normalised kept keys
    int32_t* pivot;        // [bsz * n_q_heads][q_len]
    int64_t k_stride_b, k_stride_h, k_stride_l, v_stride_b, v_stride_h, v_stride_l, out_stride_h;
    int bsz, n_q_heads, group, q_len, window, n_keep, rows;      // rows = n_keep + window
};

struct ThinkArgs {         // ThinK channel pruning (kvc_think.hip)
    const void* q;         // [bsz][n_heads][q_len][head_dim] by strides: the last 32 rows are read
    const void* kc;        // compressed keys [bsz * n_heads][rows][head_dim], kc_stride_h elements between heads, rows dense
    void* pruned;          // [bsz * n_heads][rows - recent][head_dim - n_prune]
    uint8_t* keep;         // [bsz * n_heads][head_dim]: 1 = channel kept
    void* scores;          // [bsz * n_heads][head_dim] dtype or null
    int64_t q_stride_b, q_stride_h, q_stride_l, kc_stride_h;
    int bsz, n_heads, q_len, head_dim, rows, recent, n_prune;
};

struct L2NormArgs {        // l2norm_kernel (L2NormCluster, pyramidkv_utils.py:419)
    const void* k;         // [bsz][n_kv_heads][q_len][head_dim] by strides (elements)
    void* norms;           // [bsz][n_q_heads][q_len] dtype: the norm of KV head h / group in every one of its query-head rows
    int64_t stride_b, stride_h, stride_l;
    int bsz, n_q_heads, n_kv_heads, q_len, head_dim;
};

struct RaggedArgs {        // ragged_head_stats_kernel / ragged_budget_kernel (AdaKV budgets)
    const void* scores;    // [bsz][H][n] dtype (pooled window-mean scores)
    float* ratio;          // [bsz][H] fp32 scratch: sum(top base) / sum(all) per head, dtype-rounded
    int32_t* caps;         // [bsz][H] out: rows each head keeps (without the window)
    int32_t* flags;        // [bsz][2] out: [0] cross-head tie at the global threshold, [1] slots given to threshold-valued scores
    int n, heads_per_batch, base, floor_capacity, normalize;
    float mix;             // (float)(1 - floor_ratio)
};

struct RaggedGatherArgs {  // ragged_gather_kernel: K and V rows -> the flat cache
    const void* k; const void* v; void* k_flat; void* v_flat;
    const int64_t* idx;    // [bsz*H][idx_stride] sorted indices (sort_prefix_kernel)
    const int32_t* caps;   // [bsz*H]
    const int64_t* seg_off;    // [bsz*H] first row of each head's segment in the flat cache
    int64_t k_stride_b, k_stride_h, k_stride_l, v_stride_b, v_stride_h, v_stride_l;
    int idx_stride, n_q_heads, group, q_len, window, row_bytes, esize;
};

struct RaggedDecodeArgs {  // one decode step over the ragged cache
    const void* q; const void* k_new; const void* v_new; void* k_flat; void* v_flat; void* out;
    const int64_t* seg_off; const int32_t* seg_len;      // [bsz*H]: segment start (rows) and rows after the prefill
    int64_t q_stride_b, q_stride_h, q_stride_l, new_stride_b, new_stride_h, new_stride_l, out_stride_b, out_stride_h, out_stride_l;
    int n_q_heads, group, appended, new_rows, esize, row_bytes;
    float scaling;
};

struct DecodeArgs {        // one decode step over the compacted cache (kvc_decode.hip); strides in elements
    const void* q; const void* k_new; const void* v_new;
    const void* k_prefix; const void* v_prefix;       // [b][Hq][prefix rows][D]
    void* k_tail; void* v_tail;                       // [b][Hkv][capacity][D], rows [0, tail_rows) filled
    void* out;                                        // attention output, row (b, h, i) at out + b*sb + h*sh + i*sl
    int64_t q_stride_b, q_stride_h, q_stride_l;
    int64_t new_stride_b, new_stride_h, new_stride_l;
    int64_t prefix_stride_b, prefix_stride_h, tail_stride_b, tail_stride_h;
    int64_t out_stride_b, out_stride_h, out_stride_l;
    int bsz, n_q_heads, n_kv_heads, group, prefix_rows, tail_rows, new_rows, esize, row_bytes;
    float scaling;
    // kvc_decode_step2: values with their own strides, ThinK's channel-pruned leading rows, rows split over workgroups
    int64_t vprefix_stride_b, vprefix_stride_h;
    const void* k_pruned; const int16_t* chan;        // [b][Hq][pruned_rows][pruned_dim], [b][Hq][pruned_dim]
    int64_t pruned_stride_b, pruned_stride_h, chan_stride_b, chan_stride_h;
    int pruned_rows, pruned_dim;
    float* part; int splits, rows_per_split;          // workspace: (m, l, acc[D]) per (b, h, token, split)
};

struct DecodeRowsArgs {    // kvc_decode_rows.hip: DecodeArgs (pruned_rows = 0) + the prefix rows each batch row may see
    DecodeArgs a;                                     // a.prefix_rows: what the buffers hold (the clamp of every entry)
    const int32_t* rows_b;                            // [bsz], device
};

struct DecodeDevArgs {     // kvc_decode_dev.hip: DecodeArgs (pruned_rows = 0, tail_rows unused) + the lengths the device reads
    DecodeArgs a;
    const int32_t* rows_b;                            // [bsz], device, or null: a.prefix_rows for every batch row
    const int32_t* tail_dev;                          // 1 int32, device: rows in the tail before this step
    int tail_capacity;                                // rows the tail buffers hold (the clamp of the counter)
};

struct DecodeDevRingArgs { // kvc_decode_dev.hip: DecodeDevArgs + the query ring the append launch also writes
    DecodeDevArgs d;
    void* ring;                                       // [b][Hq][ring_rows][D], rows dense: query row i -> slot (T + i) % ring_rows
    int64_t ring_stride_b, ring_stride_h;             // elements
    int ring_rows;
};

struct QuantArgs {         // kvc_quant.hip: quantize / de-quantize rows [row0, row0 + rows) of one segment (include/kvc.h layout)
    const void* src; void* dst;                       // [b][h][row][D] elements (quantize reads src, de-quantize writes dst)
    uint8_t* codes; const uint8_t* codes_in; float* meta; const float* meta_in;
    int64_t s_stride_b, s_stride_h, s_stride_l, c_stride_b, c_stride_h, m_stride_b, m_stride_h;
    int bsz, n_heads, head_dim, group, row0, rows;
};

struct QSegArgs {          // one quantized segment of the decode cache
    const uint8_t* kc; const uint8_t* vc; const float* km; const float* vm;
    int64_t c_stride_b, c_stride_h, km_stride_b, km_stride_h, vm_stride_b, vm_stride_h;
    int rows;
};

struct DecodeQArgs {       // kvc_decode_step_quant: quantized prefix + quantized tail + residual (+ the step's rows)
    const void* q; const void* k_res; const void* v_res; void* out;
    int64_t q_stride_b, q_stride_h, q_stride_l, res_stride_b, res_stride_h, out_stride_b, out_stride_h, out_stride_l;
    QSegArgs pre, qt;                                 // prefix per query head, quantized tail per KV head
    int bsz, n_q_heads, group, gsize, res_rows, new_rows;
    float scaling;
    float* part; int splits, rows_per_split;          // as DecodeArgs: (m, l, acc[D]) per (b, h, token, split)
};

struct DecodeQDevArgs {    // kvc_decode_quant_dev.hip: DecodeQArgs (qt.rows and res_rows unused) + the lengths the device reads
    DecodeQArgs a;
    const int32_t* qt_dev;                            // 1 int32, device: rows of the quantized tail in use
    const int32_t* res_dev;                           // 1 int32, device: residual rows before this step
    int qt_capacity, res_capacity;                    // rows the tail segment / the residual buffers hold (the clamps of the words)
};

struct OutlArgs {          // one outlier pool (include/kvc.h, kvc_quant_outliers) and the split threshold (already rounded to dtype)
    uint8_t* chan; void* val; int32_t* used; uint32_t* rowinfo;
    int64_t pool_stride_b, ri_stride_b, ri_stride_h;
    int pool_capacity;
    float thr;
};

struct OSegArgs {          // the key and value pools of one quantized segment, read by the decode step
    const uint8_t* kch; const uint8_t* vch; const void* kval; const void* vval; const uint32_t* kri; const uint32_t* vri;
    int64_t kpool_b, vpool_b, kri_b, kri_h, vri_b, vri_h;
    int kcap, vcap;
};
struct DecodeOArgs { OSegArgs pre, qt; };

struct DcScanArgs {        // kvc_decode_compress.hip: window scan over prefix (per query head) + tail (per KV head)
    const void* ring; const void* kp; const void* kt;  // q ring [b][Hq][W][D], prefix [b][Hq][P][D], tail [b][Hkv][T][D]
    int64_t ring_sb, ring_sh, kp_sb, kp_sh, kt_sb, kt_sh;   // elements, rows dense
    void* logits;          // [bsz*Hq][L][W] dtype (ScoreArgs layout)
    float* pmax;           // [bsz*Hq][n_parts][W] fp32
    int n_q_heads, group, prefix_rows, q_len, window, ring_start, n_parts, keys_per_part;
    float sqrt_d;
};

struct DcGatherArgs {      // two-source gather: kept row idx < P from the prefix, else from tail head h / G
    const void* src_p[2]; const void* src_t[2]; void* out[2];    // [0] keys, [1] values
    const int64_t* idx;    // [bsz*Hq][k], or null (identity: StreamingLLM)
    int64_t p_sb, p_sh, t_sb, t_sh, o_sb, o_sh;        // elements, rows dense
    int n_q_heads, group, prefix_rows, q_len, window, k, row_bytes, esize;
};

struct DecodeScoredArgs {  // kvc_decode_scored.hip: DecodeArgs (pruned_rows = 0; a.part written with one split too) + the scores
    DecodeArgs a;
    float* logit;          // [bsz*Hq][new_rows][rows] fp32 workspace: the log2-domain logit of every visible row
    float* score_prefix; float* score_tail;            // [b][Hq][capacity] fp32, running sums of attention per stored row
    int64_t sp_sb, sp_sh, st_sb, st_sh;                // floats
    int rows;              // prefix_rows + tail_rows + new_rows (launcher-set)
};

struct DecodeDevScoredArgs {   // kvc_decode_dev_scored.hip: DecodeDevArgs (d.a.part written with one split too) + the scores
    DecodeDevArgs d;
    float* logit;          // [bsz*Hq][new_rows][rows] fp32 workspace: the log2-domain logit of every visible row, by virtual row
    float* score_prefix; float* score_tail;            // [b][Hq][capacity] fp32, running sums of attention per stored row
    int64_t sp_sb, sp_sh, st_sb, st_sh;                // floats
    int rows;              // the bound prefix_rows + tail_capacity: the row stride of `logit` (launcher-set)
};

struct EvictArgs {         // kvc_decode_evict: candidate scores -> one row per head; gather of K, V and scores from two segments
    const float* score_p; const float* score_t; float* cand;     // cand [bsz*Hq][n] fp32 workspace
    float* score_out;      // [b][Hq][k + window] fp32
    const void* src_p[2]; const void* src_t[2]; void* out[2];    // [0] keys, [1] values
    const int64_t* idx;    // [bsz*Hq][k] virtual row numbers
    int64_t sp_sb, sp_sh, st_sb, st_sh, so_sb, so_sh;            // floats
    int64_t p_sb, p_sh, t_sb, t_sh, o_sb, o_sh;                  // elements, rows dense
    int n_q_heads, group, prefix_rows, n, window, k, row_bytes, esize;    // n = P + T - window candidates
};

// Raise a kernel's dynamic-LDS limit above 64 KB once per (kernel instantiation, device): `cache` is a function-local
// static array owned by the caller.  Never called again on the launch path, so launches stay graph-capturable.
struct LdsCache { size_t ok[16]; };
inline int ensure_lds(const void* func, size_t lds, LdsCache& cache) {
    if (lds <= 64 * 1024) return 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev &= 15;
    if (lds <= cache.ok[dev]) return 0;
    if (hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    cache.ok[dev] = lds;
    return 0;
}

int launch_scores(const ScoreArgs& a, int dtype, int head_dim, hipStream_t st);
int launch_h2o_scores(const H2OArgs& a, int dtype, int head_dim, hipStream_t st);
int h2o_chunk_rows(int heads, int L, int esize);
bool h2o_fused_eligible(int dtype, int L, int legacy);   // exact mode: the one-kernel form applies (workspace: permuted K instead of S)   // query rows of the exact mode's logit matrix held at a time
int launch_select(const SelectArgs& a, int dtype, int tie_mode, hipStream_t st);
size_t select_lds_bytes(int k);
int launch_select_exact(const SelectArgs& a, int dtype, void* scratch, hipStream_t st);   // tie_mode torch_cpu
size_t select_exact_scratch_bytes(int heads, int n, int k);     // per item
bool select_gather_eligible(int dtype, int n, int row_bytes, const int* keep, int n_items);   // tie_mode torch_cpu, WaveHeapL budgets
int launch_select_gather(const SelectArgs& a, int dtype, hipStream_t st);                     // select_exact + gather in one kernel (gk, gv)
int launch_gather(const GatherPair& p, hipStream_t st);
struct CamArgs {           // CAM (kvc_cam.hip)
    const void* logits; const float* rowmax; const float* rowsum;      // the scoring stage's workspace regions
    void* colmean;            // [b*Hq][L] dtype
    void* prob;               // [b*Hq][L - W - start] dtype
    void* v; const uint8_t* mask;                                       // merge: values in place, draws
    int64_t v_stride_b, v_stride_h, v_stride_l;
    int bsz, n_q_heads, q_len, window, start;
};
int launch_cam_prob(const CamArgs& a, int dtype, hipStream_t st);
int launch_cam_merge(const CamArgs& a, int dtype, int head_dim, hipStream_t st);
int launch_decode_step(DecodeArgs a, int dtype, int head_dim, hipStream_t st);
int launch_decode_append(const DecodeArgs& a, hipStream_t st);                       // the step's rows -> tail (kvc_decode.hip)
int launch_decode_combine(const DecodeArgs& a, int dtype, int head_dim, hipStream_t st);   // splits -> out (kvc_decode.hip)
int launch_decode_step_rows(DecodeRowsArgs a, int dtype, int head_dim, hipStream_t st);     // kvc_decode_rows.hip
int decode_rows_splits(int bsz, int n_q_heads, int new_rows, int rows);
int launch_decode_step_dev(DecodeDevArgs a, int dtype, int head_dim, hipStream_t st);       // kvc_decode_dev.hip
int launch_decode_step_dev_ring(DecodeDevRingArgs a, int dtype, int head_dim, hipStream_t st);
int decode_dev_splits(int bsz, int n_q_heads, int new_rows, int rows);
int launch_quantize(const QuantArgs& a, int dtype, int nbits, int mode, hipStream_t st);
int launch_dequantize(const QuantArgs& a, int dtype, int nbits, int mode, hipStream_t st);
int launch_decode_step_quant(DecodeQArgs a, int dtype, int head_dim, int nbits, const DecodeArgs& append, hipStream_t st);
int launch_decode_step_quant_dev(DecodeQDevArgs a, int dtype, int head_dim, int nbits, const DecodeArgs& append, hipStream_t st);   // kvc_decode_quant_dev.hip
int launch_quantize_outliers(const QuantArgs& a, const OutlArgs& o, int dtype, int nbits, int mode, hipStream_t st);
int launch_dequantize_outliers(const QuantArgs& a, const OutlArgs& o, int dtype, int nbits, int mode, hipStream_t st);
int launch_decode_step_quant_outliers(DecodeQArgs a, const DecodeOArgs& o, int dtype, int head_dim, int nbits, const DecodeArgs& append,
                                      hipStream_t st);
int launch_decode_step_scored(DecodeScoredArgs a, int dtype, int head_dim, hipStream_t st);   // kvc_decode_scored.hip
int launch_decode_step_dev_scored(DecodeDevScoredArgs a, int dtype, int head_dim, hipStream_t st);   // kvc_decode_dev_scored.hip
int launch_evict_scores(const EvictArgs& a, int bsz, hipStream_t st);
int launch_evict_gather(const EvictArgs& a, int bsz, hipStream_t st);
int launch_dc_scan(const DcScanArgs& a, int dtype, int head_dim, int bsz, hipStream_t st);
int launch_dc_gather(const DcGatherArgs& a, int bsz, hipStream_t st);
int decode_splits(int bsz, int n_q_heads, int new_rows, int rows);
size_t decode_part_bytes(int bsz, int n_q_heads, int new_rows, int head_dim, int splits);
int launch_sort_prefix(const RaggedSortArgs& a, int dtype, void* scratch, hipStream_t st);
int launch_l2norm(const L2NormArgs& a, int dtype, hipStream_t st);
int launch_merge(const MergeArgs& a, int dtype, hipStream_t st);
int launch_think(const ThinkArgs& a, int dtype, hipStream_t st);
size_t sort_prefix_scratch_bytes(int heads, int n);
int launch_ragged_plan(const RaggedArgs& a, int dtype, int bsz, hipStream_t st);
int launch_ragged_head_stats(const RaggedArgs& a, int dtype, int bsz, hipStream_t st);
int launch_ragged_flatten(const RaggedArgs& a, int dtype, int bsz, const int64_t* idx, void* flat, hipStream_t st);
int launch_ragged_recount(const RaggedArgs& a, int bsz, const int64_t* top, hipStream_t st);
int launch_ragged_gather(const RaggedGatherArgs& a, int rows_max, int heads, hipStream_t st);
int launch_ragged_decode(const RaggedDecodeArgs& a, int dtype, int head_dim, int heads, hipStream_t st);
static constexpr int kFuseGatherMaxK = 512;   // select_kernel gathers the rows itself up to this k

}  // namespace kvc
