// kvc_api.hip — the C-ABI of include/kvc.h: validation, workspace carving and kernel enqueue.
// Nothing here allocates device memory, synchronises, or touches the host copy of any tensor.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kvc_common.h"
#include "kvc_launch.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int esize_of(int dtype) { return dtype == KVC_FP32 ? 4 : 2; }
inline bool scoring(int method) { return method == KVC_SNAPKV || method == KVC_PYRAMIDKV || method == KVC_H2O || method == KVC_ADAKV || method == KVC_HEADKV; }
inline bool ragged(int method) { return method == KVC_ADAKV || method == KVC_HEADKV; }

struct Layout {
    size_t logits, pmax, psum, rowmax, rowsum, scores, idx, exact, total;   // H2O: logits = S [L][L], rowmax/rowsum = [L] per head
    int n_tiles, n_chunks;
    int h2o_rows;      // H2O exact mode: query rows of S in flight; 0 in fast mode (no S)
    bool has_part16;   // the psum region holds the window methods' 16-row partial sums
};

// Validation shared by every entry point.  `need_q`: the call reads q/k for scoring.
int validate(const kvc_params* p, bool need_scores) {
    if (!p) return fail(KVC_ERR_INVALID, "params is NULL");
    if (p->method < KVC_SNAPKV || p->method > KVC_HEADKV) return fail(KVC_ERR_INVALID, "unknown method %d", p->method);
    if (p->dtype < KVC_BF16 || p->dtype > KVC_FP32) return fail(KVC_ERR_INVALID, "unknown dtype %d", p->dtype);
    if (p->bsz < 1 || p->n_q_heads < 1 || p->n_kv_heads < 1) return fail(KVC_ERR_INVALID, "bsz / head counts must be positive");
    if (p->n_q_heads % p->n_kv_heads) return fail(KVC_ERR_INVALID, "n_q_heads %d not a multiple of n_kv_heads %d", p->n_q_heads, p->n_kv_heads);
    if (p->window < 1) return fail(KVC_ERR_INVALID, "window must be >= 1");
    if (p->q_len <= p->window) return fail(KVC_ERR_INVALID, "q_len %d must exceed window %d", p->q_len, p->window);
    if (p->k < 0 || p->k > p->q_len - p->window)
        return fail(KVC_ERR_INVALID, "k=%d outside [0, q_len-window=%d] (reference: topk k out of range)", p->k, p->q_len - p->window);
    const int es = esize_of(p->dtype);
    if (p->head_dim < 1 || (p->head_dim * es) % 16) return fail(KVC_ERR_UNSUPPORTED, "head_dim*esize must be a multiple of 16 bytes");
    if (p->head_dim * es > 4096) return fail(KVC_ERR_UNSUPPORTED, "head_dim too large");
    if (p->tie_mode != KVC_TIES_TORCH_CPU && p->tie_mode != KVC_TIES_CANONICAL) return fail(KVC_ERR_INVALID, "unknown tie_mode %d", p->tie_mode);
    if (p->dot_mode != KVC_DOT_EXACT && p->dot_mode != KVC_DOT_MFMA16) return fail(KVC_ERR_INVALID, "unknown dot_mode %d", p->dot_mode);
    if (need_scores && scoring(p->method)) {
        if (p->head_dim != 64 && p->head_dim != 128) return fail(KVC_ERR_UNSUPPORTED, "scoring kernels are built for head_dim 64 and 128, got %d", p->head_dim);
        if (p->window > 64) return fail(KVC_ERR_UNSUPPORTED, "scoring window %d > 64 not built", p->window);
        if (p->method != KVC_H2O) {
            if (p->pooling != KVC_POOL_AVG && p->pooling != KVC_POOL_MAX && p->pooling != KVC_POOL_NONE)
                return fail(KVC_ERR_INVALID, "Pooling method not supported");   // pyramidkv_utils.py:333
            if (p->pooling != KVC_POOL_NONE) {
                if (p->kernel_size < 1 || p->kernel_size > 63) return fail(KVC_ERR_UNSUPPORTED, "kernel_size %d outside [1,63]", p->kernel_size);
                if ((p->kernel_size & 1) == 0)
                    return fail(KVC_ERR_UNSUPPORTED, "even kernel_size %d: the reference's pooled length becomes n+1 and its gather can index out of range", p->kernel_size);
            }
        }
    }
    return KVC_OK;
}

int check_strides(const char* what, int es, int64_t sb, int64_t sh, int64_t sl, const void* ptr) {
    if (((uintptr_t)ptr) % 16) return fail(KVC_ERR_ALIGNMENT, "%s pointer not 16-byte aligned", what);
    if ((sb * es) % 16 || (sh * es) % 16 || (sl * es) % 16) return fail(KVC_ERR_ALIGNMENT, "%s strides not multiples of 16 bytes", what);
    return KVC_OK;
}

Layout carve(const kvc_params* p, int n_items = 1) {
    Layout l;
    std::memset(&l, 0, sizeof(l));
    const size_t es = (size_t)esize_of(p->dtype);
    const size_t heads = (size_t)p->bsz * p->n_q_heads, L = (size_t)p->q_len, W = (size_t)p->window, n = L - W;
    // logits_kernel: 4 waves per workgroup, each wave walks 32-key tiles.  A call owns few KV heads: spread each head
    // over many workgroups (one tile per wave at 8k).  A batch has parallelism to spare: pick the workgroups per head so
    // that the grid is a whole number of "rounds" of the chip (3 workgroups x 256 CUs resident at once) with as many
    // tiles per wave as that allows — fewer prologues (Q image, first-tile latency), no half-empty last round
    // (measured at C2 x 32 layers: 4 tiles per wave 199-204 us, 11: 189 us, 21 = one round: 187 us, 32: 196 us).
    {
        const int tiles32 = (int)((L + 31) / 32);
        const int64_t units = (int64_t)n_items * p->bsz * p->n_kv_heads;        // workgroups per "group" index
        const int64_t slots = 3 * 256;
        int best_g = 1;
        double best = 1e30;
        const int g_max = (tiles32 + 3) / 4;
        for (int g = 1; g <= g_max; ++g) {
            const int64_t rounds = (g * units + slots - 1) / slots;
            const int tpw = (tiles32 + 4 * g - 1) / (4 * g);
            const double cost = (double)rounds * (tpw + 1.5);                   // 1.5 tiles' worth of prologue per workgroup
            if (cost < best - 1e-9) { best = cost; best_g = g; }
        }
        l.n_tiles = best_g;                                // workgroups (4 waves each) per KV head == tile maxima per row
    }
    l.n_chunks = (int)((L + 255) / 256);
    size_t off = 0;
    if (scoring(p->method)) {
        const size_t R = p->method == KVC_H2O ? L : W;     // query rows that score
        const bool h2o_fast = p->method == KVC_H2O && p->dot_mode == KVC_DOT_MFMA16 && p->dtype != KVC_FP32;
        l.h2o_rows = (p->method == KVC_H2O && !h2o_fast) ? kvc::h2o_chunk_rows((int)heads, (int)L, (int)es) : 0;
        if (l.h2o_rows > 512 && (p->debug_stage_mask & 128)) l.h2o_rows = 512;      // testing aid: several chunks at small L
        // logits: [h][L][W] for the window methods; H2O exact: the chunk [h][h2o_rows][L]; H2O fast: nothing
        // (H2O exact, fused form: the same region holds the permuted copy of K, [bsz * Hkv][L][D])
        const size_t h2o_kt = (size_t)p->bsz * p->n_kv_heads * ((L + 15) / 16 * 16) * p->head_dim * es;
        const size_t h2o_s = heads * (size_t)l.h2o_rows * L * es;
        const bool h2o_fused = p->method == KVC_H2O && !h2o_fast && kvc::h2o_fused_eligible(p->dtype, (int)L, (p->debug_stage_mask & 2048) ? 1 : 0);
        l.logits = off; off = align_up(off + (p->method == KVC_H2O ? (h2o_fast ? 0 : (h2o_fused ? h2o_kt : h2o_s)) : heads * L * R * es), 256);
        l.pmax = off;   off = align_up(off + (p->method == KVC_H2O ? 0 : heads * (size_t)l.n_tiles * W * 4), 256);
        // H2O: column sums of every 256-row block (+ one slot for the leftover rows), fp32, columns padded to even
        // window methods at W = 16 / 32 / 64, 16-bit: the 16-row partial window sums of softmax_rows16_kernel, fp32
        l.has_part16 = p->method != KVC_H2O && p->dtype != KVC_FP32 && (W == 16 || W == 32 || W == 64);
        l.psum = off;   off = align_up(off + ((p->method == KVC_H2O && !h2o_fast) ? heads * (size_t)(l.n_chunks + 1) * ((n + 1) & ~(size_t)1) * 4
                                              : (l.has_part16 ? heads * (W / 16) * ((n + 1) & ~(size_t)1) * 4 : 0)), 256);
        l.rowmax = off; off = align_up(off + heads * R * 4, 256);
        l.rowsum = off; off = align_up(off + heads * R * 4, 256);
        l.scores = off; off = align_up(off + heads * n * es, 256);
        l.idx = off;    off = align_up(off + heads * (size_t)p->k * 8, 256);
        l.exact = off;     // (the exact tie mode's scratch follows the per-item regions: exact_scratch_total)
    }
    l.total = off;
    return l;
}

int check_ws(const Layout& l, void* ws, size_t bytes) {
    if (l.total == 0) return KVC_OK;
    if (!ws) return fail(KVC_ERR_WORKSPACE, "workspace is NULL, need %zu bytes", l.total);
    if (((uintptr_t)ws) % 256) return fail(KVC_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    if (bytes < l.total) return fail(KVC_ERR_WORKSPACE, "workspace too small: %zu < %zu", bytes, l.total);
    return KVC_OK;
}

int hip_ok(const char* where) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(KVC_ERR_HIP, "%s: %s", where, hipGetErrorString(e));
    return KVC_OK;
}

// One "item" = one update_kv (one layer).  kvc_compress is the 1-item case of the batched entry point.
struct Items {
    int n;
    const void* q[kvc::KVC_MAX_ITEMS]; const void* k[kvc::KVC_MAX_ITEMS]; const void* v[kvc::KVC_MAX_ITEMS];
    void* k_out[kvc::KVC_MAX_ITEMS]; void* v_out[kvc::KVC_MAX_ITEMS];
    void* scores[kvc::KVC_MAX_ITEMS]; int64_t* idx[kvc::KVC_MAX_ITEMS];
    int keep[kvc::KVC_MAX_ITEMS];
    int64_t out_stride_h[kvc::KVC_MAX_ITEMS];       // elements between output heads, 0 = dense
    int k_max;
};

// scores for every item (pointers in it.scores must be set).  Workspace of item i = ws + i * l.total.
int enqueue_scores(const kvc_params* p, const Layout& l, const Items& it, char* ws, hipStream_t st) {
    if (p->method == KVC_H2O) {
        for (int i = 0; i < it.n; ++i) {
            char* w = ws + (size_t)i * l.total;
            kvc::H2OArgs h;
            h.q = it.q[i]; h.k = it.k[i];
            h.S = w + l.logits;
            h.row0 = 0; h.rows = p->q_len; h.s_rows = l.h2o_rows;
            h.fast = l.h2o_rows == 0 ? 1 : 0;
            h.kt = w + l.logits;
            h.legacy = (p->debug_stage_mask & 2048) ? 1 : 0;
            h.rowmax = reinterpret_cast<float*>(w + l.rowmax);
            h.rinv = reinterpret_cast<float*>(w + l.rowsum);
            h.part = reinterpret_cast<float*>(w + l.psum);
            h.scores = it.scores[i];
            h.q_stride_b = p->q_stride_b; h.q_stride_h = p->q_stride_h; h.q_stride_l = p->q_stride_l;
            h.k_stride_b = p->k_stride_b; h.k_stride_h = p->k_stride_h; h.k_stride_l = p->k_stride_l;
            h.bsz = p->bsz; h.n_q_heads = p->n_q_heads; h.n_kv_heads = p->n_kv_heads; h.group = p->n_q_heads / p->n_kv_heads;
            h.q_len = p->q_len; h.window = p->window;
            h.sqrt_d = (float)std::sqrt((double)p->head_dim);
            const int rc = kvc::launch_h2o_scores(h, p->dtype, p->head_dim, st);
            if (rc) return fail(rc, "no H2O kernel for dtype %d head_dim %d", p->dtype, p->head_dim);
        }
        return hip_ok("h2o scores launch");
    }
    kvc::ScoreArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int i = 0; i < it.n; ++i) { a.q.p[i] = it.q[i]; a.k.p[i] = it.k[i]; a.scores.p[i] = it.scores[i]; }
    a.n_items = it.n;
    a.ws = ws; a.ws_item_stride = (int64_t)l.total;
    a.off_logits = (int64_t)l.logits; a.off_pmax = (int64_t)l.pmax;
    a.off_rowmax = (int64_t)l.rowmax; a.off_rowsum = (int64_t)l.rowsum;
    a.off_part16 = l.has_part16 ? (int64_t)l.psum : -1;
    a.q_stride_b = p->q_stride_b; a.q_stride_h = p->q_stride_h; a.q_stride_l = p->q_stride_l;
    a.k_stride_b = p->k_stride_b; a.k_stride_h = p->k_stride_h; a.k_stride_l = p->k_stride_l;
    a.bsz = p->bsz; a.n_q_heads = p->n_q_heads; a.n_kv_heads = p->n_kv_heads;
    a.group = p->n_q_heads / p->n_kv_heads;
    a.q_len = p->q_len; a.window = p->window;
    a.n_tiles = l.n_tiles;
    a.kernel_size = p->kernel_size; a.pooling = p->pooling;
    a.stage_mask = p->debug_stage_mask;
    a.fast_dot = (p->dot_mode == KVC_DOT_MFMA16 && p->dtype != KVC_FP32) ? 1 : 0;
    a.window_mean = ragged(p->method) ? 1 : 0;              // calcul_attn_sore (:660): .mean(dim=-2)
    a.dbg = nullptr;
#if defined(KVC_STAMPS)
    a.dbg = reinterpret_cast<unsigned long long*>(it.scores[0]);   // diagnostic build: stamps land in scores_out
    if ((p->debug_stage_mask & 7) == 6 && it.idx[0]) a.dbg = reinterpret_cast<unsigned long long*>(it.idx[0]);   // softmax stamps: item 0's idx_out
#endif
    a.sqrt_d = (float)std::sqrt((double)p->head_dim);   // math.sqrt(head_dim) -> fp32 (pyramidkv_utils.py:317)
    const int rc = kvc::launch_scores(a, p->dtype, p->head_dim, st);
    if (rc) return fail(rc, "no scoring kernel for dtype %d head_dim %d", p->dtype, p->head_dim);
    return hip_ok("scores launch");
}

// which: 0 = K (it.k -> it.k_out), 1 = V.  use_idx: gather through it.idx (else identity indices, StreamingLLM).
kvc::GatherArgs gather_args(const kvc_params* p, const Items& it, int which, bool use_idx) {
    kvc::GatherArgs g;
    std::memset(&g, 0, sizeof(g));
    for (int i = 0; i < it.n; ++i) {
        g.src.p[i] = which ? it.v[i] : it.k[i];
        g.out.p[i] = which ? it.v_out[i] : it.k_out[i];
        g.idx.p[i] = use_idx ? it.idx[i] : nullptr;
        g.k.v[i] = it.keep[i];
        g.out_head_bytes.v[i] = it.out_stride_h[i] * esize_of(p->dtype);
    }
    g.n_items = it.n; g.k_max = it.k_max;
    g.stride_b = which ? p->v_stride_b : p->k_stride_b;
    g.stride_h = which ? p->v_stride_h : p->k_stride_h;
    g.stride_l = which ? p->v_stride_l : p->k_stride_l;
    g.bsz = p->bsz; g.n_q_heads = p->n_q_heads; g.group = p->n_q_heads / p->n_kv_heads;
    g.q_len = p->q_len; g.window = p->window;
    g.esize = esize_of(p->dtype);
    g.row_bytes = p->head_dim * g.esize;
    return g;
}

// A7 for every item (+ A8 in the same kernel when `fuse`).  exact_scratch: n_items regions for the exact tie mode.
int enqueue_select(const kvc_params* p, const Items& it, bool fuse, void* exact_scratch, hipStream_t st, bool members_only = false) {
    const int n_sel = p->q_len - p->window;
    if (p->tie_mode == KVC_TIES_CANONICAL) {
        if (it.k_max > 16384) return fail(KVC_ERR_UNSUPPORTED, "tie_mode canonical: k=%d > 16384 (the LDS sort of the selected set) not built", it.k_max);
        if (n_sel > 131072) return fail(KVC_ERR_UNSUPPORTED, "tie_mode canonical: more than 131072 candidates per head not built (torch_cpu has no such limit)");
    } else if ((int64_t)it.k_max * 64 <= (int64_t)n_sel && it.k_max > 18000) {
        return fail(KVC_ERR_UNSUPPORTED, "tie_mode torch_cpu: a partial_sort heap of k=%d does not fit in LDS", it.k_max);
    }
    kvc::SelectArgs s;
    std::memset(&s, 0, sizeof(s));
    for (int i = 0; i < it.n; ++i) { s.scores.p[i] = it.scores[i]; s.idx.p[i] = it.idx[i]; s.k.v[i] = it.keep[i]; }
    s.n_items = it.n;
    s.n = p->q_len - p->window; s.k_max = it.k_max; s.heads = p->bsz * p->n_q_heads;
    s.pow2 = 1;
    while (s.pow2 < s.k_max) s.pow2 <<= 1;
    if (fuse) { s.fuse = 1; s.gk = gather_args(p, it, 0, true); s.gv = gather_args(p, it, 1, true); }
    s.members_only = members_only ? 1 : 0;
    if (p->tie_mode == KVC_TIES_TORCH_CPU) {
        if (fuse) {                                          // the caller checked kvc::select_gather_eligible
            const int rc = kvc::launch_select_gather(s, p->dtype, st);
            if (rc) return fail(rc, "exact select + gather launch failed");
            return hip_ok("exact select + gather launch");
        }
#if defined(KVC_STAMPS)
        if (p->debug_stage_mask & 32) s.fuse = 2;            // diag build: phase stamps over the index output (no gather follows)
#endif
        const int rc = kvc::launch_select_exact(s, p->dtype, exact_scratch, st);
        if (rc == KVC_ERR_WORKSPACE) return fail(rc, "tie_mode torch_cpu at n=%d needs the workspace (kvc_workspace_bytes)", s.n);
        if (rc) return fail(rc, "exact select launch failed");
        return hip_ok("exact select launch");
    }
    const int rc = kvc::launch_select(s, p->dtype, p->tie_mode, st);
    if (rc == KVC_ERR_UNSUPPORTED) return fail(rc, "tie_mode %d not built for this shape", p->tie_mode);
    if (rc) return fail(rc, "select launch failed");
    return hip_ok("select launch");
}

int enqueue_gather(const kvc::GatherArgs* g0, const kvc::GatherArgs* g1, hipStream_t st) {
    kvc::GatherPair pr;
    pr.t[0] = *g0;
    pr.count = 1;
    if (g1) { pr.t[1] = *g1; pr.count = 2; } else { pr.t[1] = *g0; }
    kvc::launch_gather(pr, st);
    return hip_ok("gather launch");
}

// Bytes of the (shared, after the per-item regions) scratch the exact tie mode needs for all items.
size_t exact_scratch_total(const kvc_params* p, int n_items, const int* keep) {
    if (p->tie_mode != KVC_TIES_TORCH_CPU || !scoring(p->method)) return 0;
    size_t worst = 0;
    for (int i = 0; i < n_items; ++i) {
        const size_t b = kvc::select_exact_scratch_bytes(p->bsz * p->n_q_heads, p->q_len - p->window, keep[i]);
        if (b > worst) worst = b;
    }
    return align_up(worst * (size_t)n_items, 256);
}

// The whole pipeline for it.n items of identical shape (p) and per-item k.
int run_items(const kvc_params* p, Items& it, void* workspace, size_t workspace_bytes, hipStream_t st) {
    const int es = esize_of(p->dtype);
    if (int rc = check_strides("k", es, p->k_stride_b, p->k_stride_h, p->k_stride_l, it.k[0])) return rc;
    if (int rc = check_strides("v", es, p->v_stride_b, p->v_stride_h, p->v_stride_l, it.v[0])) return rc;
    it.k_max = 0;
    for (int i = 0; i < it.n; ++i) {
        if (!it.k[i] || !it.v[i] || !it.k_out[i] || !it.v_out[i]) return fail(KVC_ERR_INVALID, "k, v, k_out and v_out must be non-NULL (item %d)", i);
        if (((uintptr_t)it.k[i]) % 16 || ((uintptr_t)it.v[i]) % 16 || ((uintptr_t)it.k_out[i]) % 16 || ((uintptr_t)it.v_out[i]) % 16)
            return fail(KVC_ERR_ALIGNMENT, "k / v / k_out / v_out not 16-byte aligned (item %d)", i);
        if (it.keep[i] < 0 || it.keep[i] > p->q_len - p->window) return fail(KVC_ERR_INVALID, "k=%d outside [0, q_len-window] (item %d)", it.keep[i], i);
        if (it.keep[i] > it.k_max) it.k_max = it.keep[i];
    }
    for (int i = 0; i < it.n; ++i) {
        const int64_t os = it.out_stride_h[i];
        if (os == 0) continue;
        if (os < (int64_t)(it.keep[i] + p->window) * p->head_dim)
            return fail(KVC_ERR_INVALID, "out_stride_h %lld smaller than (k + window) * head_dim = %lld (item %d)", (long long)os,
                        (long long)(it.keep[i] + p->window) * p->head_dim, i);
        if ((os * es) % 16) return fail(KVC_ERR_ALIGNMENT, "out_stride_h not a multiple of 16 bytes (item %d)", i);
    }
    if (!scoring(p->method)) {
        for (int i = 0; i < it.n; ++i)
            if (it.idx[i] && it.keep[i] > 0)
                return fail(KVC_ERR_UNSUPPORTED, "StreamingLLM: idx_out must be NULL (indices are arange(k), pyramidkv_utils.py:607)");
        const kvc::GatherArgs gk = gather_args(p, it, 0, false), gv = gather_args(p, it, 1, false);
        return enqueue_gather(&gk, &gv, st);
    }
    kvc_params pk = *p;
    pk.k = it.k_max;
    const Layout l = carve(&pk, it.n);
    const size_t exact = exact_scratch_total(p, it.n, it.keep);
    const size_t need = l.total * (size_t)it.n + exact;
    if (!workspace) return fail(KVC_ERR_WORKSPACE, "workspace is NULL, need %zu bytes", need);
    if (((uintptr_t)workspace) % 256) return fail(KVC_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    if (workspace_bytes < need) return fail(KVC_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, need);
    char* ws = static_cast<char*>(workspace);
    bool any_zero = false;
    for (int i = 0; i < it.n; ++i) {
        if (!it.q[i]) return fail(KVC_ERR_INVALID, "q must be non-NULL for scoring methods (item %d)", i);
        if (((uintptr_t)it.q[i]) % 16) return fail(KVC_ERR_ALIGNMENT, "q pointer not 16-byte aligned (item %d)", i);
        if (it.idx[i] && ((uintptr_t)it.idx[i]) % 16) return fail(KVC_ERR_ALIGNMENT, "idx_out not 16-byte aligned");
        if (it.scores[i] && ((uintptr_t)it.scores[i]) % 16) return fail(KVC_ERR_ALIGNMENT, "scores_out not 16-byte aligned");
        char* w = ws + (size_t)i * l.total;
        if (!it.scores[i]) it.scores[i] = w + l.scores;
        if (!it.idx[i]) it.idx[i] = reinterpret_cast<int64_t*>(w + l.idx);
        any_zero = any_zero || it.keep[i] == 0;
    }
    if (int rc = check_strides("q", es, p->q_stride_b, p->q_stride_h, p->q_stride_l, it.q[0])) return rc;
    if (any_zero && it.n > 1) return fail(KVC_ERR_UNSUPPORTED, "a batch needs k >= 1 for every item");
    const int dbg = p->debug_stage_mask;
    if (!(dbg & 96))                                         // profiling aid bits 5 / 6: scores (and indices) of the previous run
        if (int rc = enqueue_scores(p, l, it, ws, st)) return rc;
    if ((dbg & 7) != 0) return KVC_OK;                       // profiling aid: only the selected scoring kernels
    if (dbg & 64) {                                          // ... only the gather
        const kvc::GatherArgs gk = gather_args(p, it, 0, true), gv = gather_args(p, it, 1, true);
        return enqueue_gather(&gk, &gv, st);
    }
    if (it.k_max == 0) {                                     // nothing to select: only the window tail is kept
        const kvc::GatherArgs gk = gather_args(p, it, 0, false), gv = gather_args(p, it, 1, false);
        return enqueue_gather(&gk, &gv, st);
    }
    // the gather rides in the selecting kernel: canonical ties up to kFuseGatherMaxK; torch_cpu ties when every item takes
    // WaveHeapL (debug_stage_mask bit 13: the separate select_exact + gather launches instead, identical results)
    bool fuse = it.k_max <= kvc::kFuseGatherMaxK && p->tie_mode == KVC_TIES_CANONICAL;
    if (p->tie_mode == KVC_TIES_TORCH_CPU && !(dbg & 8192))
        fuse = kvc::select_gather_eligible(p->dtype, p->q_len - p->window, p->head_dim * es, it.keep, it.n);
#if defined(KVC_STAMPS)
    if (dbg & 32) fuse = fuse && p->tie_mode == KVC_TIES_CANONICAL;     // stamps in the index output: the separate select_exact
#endif
    if (int rc = enqueue_select(p, it, fuse, ws + l.total * (size_t)it.n, st)) return rc;
    if (fuse) return KVC_OK;
#if defined(KVC_STAMPS)
    if (dbg & 32) return KVC_OK;                             // the index output holds phase stamps in this build: no gather
#endif
    const kvc::GatherArgs gk = gather_args(p, it, 0, true), gv = gather_args(p, it, 1, true);
    return enqueue_gather(&gk, &gv, st);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int kvc_version(void) { return KVC_VERSION; }

__attribute__((visibility("default"))) const char* kvc_last_error(void) { return g_err; }

__attribute__((visibility("default"))) size_t kvc_workspace_bytes(const kvc_params* p) {
    if (validate(p, true) != KVC_OK) return 0;
    g_err[0] = 0;
    return carve(p).total + exact_scratch_total(p, 1, &p->k);
}

__attribute__((visibility("default"))) size_t kvc_workspace_bytes_batch(const kvc_params* p, int n_items, const int32_t* k_per_item) {
    if (validate(p, true) != KVC_OK) return 0;
    if (n_items < 1 || !k_per_item) { fail(KVC_ERR_INVALID, "n_items must be >= 1 and k_per_item non-NULL"); return 0; }
    // kvc_compress_batch runs chunks of KVC_MAX_ITEMS items one after the other in the same workspace: size the largest
    size_t need = 0;
    for (int base = 0; base < n_items; base += kvc::KVC_MAX_ITEMS) {
        const int n = n_items - base < kvc::KVC_MAX_ITEMS ? n_items - base : kvc::KVC_MAX_ITEMS;
        kvc_params pk = *p;
        pk.k = 0;
        for (int i = 0; i < n; ++i) {
            const int kk = k_per_item[base + i];
            if (kk < 0 || kk > p->q_len - p->window) { fail(KVC_ERR_INVALID, "k=%d out of range (item %d)", kk, base + i); return 0; }
            if (kk > pk.k) pk.k = kk;
        }
        const size_t b = carve(&pk, n).total * (size_t)n + exact_scratch_total(p, n, k_per_item + base);
        if (b > need) need = b;
    }
    g_err[0] = 0;
    return need;
}

__attribute__((visibility("default"))) int kvc_workspace_layout(const kvc_params* p, size_t offs[3]) {
    if (int rc = validate(p, true)) return rc;
    if (!offs) return fail(KVC_ERR_INVALID, "offs is NULL");
    const Layout l = carve(p);
    offs[0] = l.logits; offs[1] = l.rowmax; offs[2] = l.rowsum;
    return KVC_OK;
}

__attribute__((visibility("default"))) int64_t kvc_pyramid_k(int64_t cap, int64_t W, int64_t q_len, int64_t layer_idx,
                                                              int64_t n_layers, int64_t beta) {
    // pyramidkv_utils.py:205-215 (Python floor division restated for possibly negative operands)
    int64_t min_num = (cap - W) / beta;
    if (((cap - W) % beta != 0) && (((cap - W) < 0) != (beta < 0))) --min_num;
    int64_t max_num = (cap - W) * 2 - min_num;
    if (max_num >= q_len - W) { max_num = q_len - W; min_num = (cap - W) * 2 - max_num; }
    const int64_t num = max_num - min_num, den = n_layers - 1;
    int64_t steps = 0;
    if (den != 0) { steps = num / den; if ((num % den != 0) && ((num < 0) != (den < 0))) --steps; }
    if (q_len < cap) return -1;                       // :218 pass-through
    if (q_len < (cap - W) * 2) return cap - W;        // :220 SnapKV budget
    return max_num - layer_idx * steps;               // :252
}

__attribute__((visibility("default"))) int kvc_scores(const kvc_params* p, const void* q, const void* k, void* scores_out,
                                                      void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = validate(p, true)) return rc;
    if (!scoring(p->method)) return fail(KVC_ERR_INVALID, "StreamingLLM has no scores");
    if (!q || !k || !scores_out) return fail(KVC_ERR_INVALID, "q, k and scores_out must be non-NULL");
    const int es = esize_of(p->dtype);
    if (int rc = check_strides("q", es, p->q_stride_b, p->q_stride_h, p->q_stride_l, q)) return rc;
    if (int rc = check_strides("k", es, p->k_stride_b, p->k_stride_h, p->k_stride_l, k)) return rc;
    if (((uintptr_t)scores_out) % 16) return fail(KVC_ERR_ALIGNMENT, "scores_out not 16-byte aligned");
    const Layout l = carve(p);
    if (int rc = check_ws(l, workspace, workspace_bytes)) return rc;
    Items it;
    std::memset(&it, 0, sizeof(it));
    it.n = 1; it.q[0] = q; it.k[0] = k; it.scores[0] = scores_out;
    return enqueue_scores(p, l, it, static_cast<char*>(workspace), static_cast<hipStream_t>(hip_stream));
}

__attribute__((visibility("default"))) size_t kvc_select_workspace_bytes(const kvc_params* p) {
    if (validate(p, false) != KVC_OK) return 0;
    g_err[0] = 0;
    if (p->tie_mode != KVC_TIES_TORCH_CPU || p->k == 0) return 0;
    return align_up(kvc::select_exact_scratch_bytes(p->bsz * p->n_q_heads, p->q_len - p->window, p->k), 256);
}

__attribute__((visibility("default"))) int kvc_select(const kvc_params* p, const void* scores, int64_t* idx_out,
                                                      void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = validate(p, false)) return rc;
    if (!scores || !idx_out) return fail(KVC_ERR_INVALID, "scores and idx_out must be non-NULL");
    if (((uintptr_t)scores) % 16 || ((uintptr_t)idx_out) % 16) return fail(KVC_ERR_ALIGNMENT, "scores / idx_out not 16-byte aligned");
    if (p->k == 0) return KVC_OK;
    void* scratch = nullptr;
    if (p->tie_mode == KVC_TIES_TORCH_CPU) {
        const size_t need = kvc::select_exact_scratch_bytes(p->bsz * p->n_q_heads, p->q_len - p->window, p->k);
        if (need) {
            if (!workspace || workspace_bytes < need || ((uintptr_t)workspace) % 256)
                return fail(KVC_ERR_WORKSPACE, "kvc_select with tie_mode torch_cpu needs %zu bytes of 256-byte aligned workspace", need);
            scratch = workspace;
        }
    }
    Items it;
    std::memset(&it, 0, sizeof(it));
    it.n = 1; it.scores[0] = const_cast<void*>(scores); it.idx[0] = idx_out; it.keep[0] = p->k; it.k_max = p->k;
    return enqueue_select(p, it, false, scratch, static_cast<hipStream_t>(hip_stream));
}

__attribute__((visibility("default"))) int kvc_gather(const kvc_params* p, const void* src, int64_t stride_b, int64_t stride_h,
                                                      int64_t stride_l, const int64_t* idx, void* out, void* hip_stream) {
    if (int rc = validate(p, false)) return rc;
    if (!src || !out) return fail(KVC_ERR_INVALID, "src and out must be non-NULL");
    if (int rc = check_strides("src", esize_of(p->dtype), stride_b, stride_h, stride_l, src)) return rc;
    if (((uintptr_t)out) % 16) return fail(KVC_ERR_ALIGNMENT, "out not 16-byte aligned");
    Items it;
    std::memset(&it, 0, sizeof(it));
    it.n = 1; it.k[0] = src; it.k_out[0] = out; it.idx[0] = const_cast<int64_t*>(idx); it.keep[0] = p->k; it.k_max = p->k;
    it.out_stride_h[0] = p->out_stride_h;
    kvc_params ps = *p;
    ps.k_stride_b = stride_b; ps.k_stride_h = stride_h; ps.k_stride_l = stride_l;
    const kvc::GatherArgs g = gather_args(&ps, it, 0, idx != nullptr);
    return enqueue_gather(&g, nullptr, static_cast<hipStream_t>(hip_stream));
}

namespace {
int decode_check(const kvc_decode_params* p, const kvc_decode_ext* x) {
    if (!p) return fail(KVC_ERR_INVALID, "params is NULL");
    if (p->dtype < KVC_BF16 || p->dtype > KVC_FP32) return fail(KVC_ERR_INVALID, "unknown dtype %d", p->dtype);
    if (p->bsz < 1 || p->n_q_heads < 1 || p->n_kv_heads < 1 || p->n_q_heads % p->n_kv_heads)
        return fail(KVC_ERR_INVALID, "bsz / head counts invalid");
    if (p->head_dim != 64 && p->head_dim != 128) return fail(KVC_ERR_UNSUPPORTED, "decode kernels are built for head_dim 64 and 128, got %d", p->head_dim);
    if (p->prefix_rows < 0 || p->tail_rows < 0 || p->new_rows < 1) return fail(KVC_ERR_INVALID, "row counts invalid");
    if (x) {
        if (x->pruned_rows < 0) return fail(KVC_ERR_INVALID, "pruned_rows < 0");
        if (x->pruned_rows > 0 && (x->pruned_dim < 1 || x->pruned_dim > p->head_dim || (x->pruned_dim * esize_of(p->dtype)) % 16))
            return fail(KVC_ERR_INVALID, "pruned_dim must be 1..head_dim and a multiple of 16 bytes (pad the kept channels with zero columns), got %d", x->pruned_dim);
    }
    return KVC_OK;
}
int decode_run(const kvc_decode_params* p, const kvc_decode_ext* x, const void* q, const void* k_new, const void* v_new,
               const void* k_prefix, const void* v_prefix, void* k_tail, void* v_tail, const void* k_pruned, const int16_t* chan,
               void* out, void* workspace, size_t workspace_bytes, void* hip_stream, const int32_t* rows_b = nullptr, bool per_row = false) {
    if (int rc = decode_check(p, x)) return rc;
    if (per_row && !rows_b) return fail(KVC_ERR_INVALID, "prefix_rows_b is NULL");
    if (per_row && ((uintptr_t)rows_b) % 4) return fail(KVC_ERR_ALIGNMENT, "prefix_rows_b is not 4-byte aligned");
    const int pruned = x ? x->pruned_rows : 0;
    if (!q || !k_new || !v_new || !k_tail || !v_tail || !out || (p->prefix_rows > 0 && !k_prefix) || (p->prefix_rows + pruned > 0 && !v_prefix))
        return fail(KVC_ERR_INVALID, "q, k_new, v_new, the tail, out (and the prefix when it has rows) must be non-NULL");
    if (pruned > 0 && (!k_pruned || !chan)) return fail(KVC_ERR_INVALID, "pruned_rows > 0 needs k_pruned and chan");
    const int es = esize_of(p->dtype);
    const void* ptrs[] = {q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, pruned > 0 ? k_pruned : nullptr};
    for (const void* ptr : ptrs) if (((uintptr_t)ptr) % 16) return fail(KVC_ERR_ALIGNMENT, "a pointer is not 16-byte aligned");
    const int64_t strides[] = {p->q_stride_b, p->q_stride_h, p->q_stride_l, p->new_stride_b, p->new_stride_h, p->new_stride_l,
                               p->prefix_stride_b, p->prefix_stride_h, p->tail_stride_b, p->tail_stride_h,
                               x ? x->v_prefix_stride_b : 0, x ? x->v_prefix_stride_h : 0, pruned > 0 ? x->pruned_stride_b : 0, pruned > 0 ? x->pruned_stride_h : 0};
    for (int64_t sd : strides) if ((sd * es) % 16) return fail(KVC_ERR_ALIGNMENT, "a stride is not a multiple of 16 bytes");
    kvc::DecodeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.q = q; a.k_new = k_new; a.v_new = v_new; a.k_prefix = k_prefix; a.v_prefix = v_prefix; a.k_tail = k_tail; a.v_tail = v_tail; a.out = out;
    a.q_stride_b = p->q_stride_b; a.q_stride_h = p->q_stride_h; a.q_stride_l = p->q_stride_l;
    a.new_stride_b = p->new_stride_b; a.new_stride_h = p->new_stride_h; a.new_stride_l = p->new_stride_l;
    a.prefix_stride_b = p->prefix_stride_b; a.prefix_stride_h = p->prefix_stride_h;
    a.vprefix_stride_b = (x && x->v_prefix_stride_h) ? x->v_prefix_stride_b : p->prefix_stride_b;
    a.vprefix_stride_h = (x && x->v_prefix_stride_h) ? x->v_prefix_stride_h : p->prefix_stride_h;
    a.tail_stride_b = p->tail_stride_b; a.tail_stride_h = p->tail_stride_h;
    a.out_stride_b = p->out_stride_b; a.out_stride_h = p->out_stride_h; a.out_stride_l = p->out_stride_l;
    a.bsz = p->bsz; a.n_q_heads = p->n_q_heads; a.n_kv_heads = p->n_kv_heads; a.group = p->n_q_heads / p->n_kv_heads;
    a.prefix_rows = p->prefix_rows; a.tail_rows = p->tail_rows; a.new_rows = p->new_rows;
    a.esize = es; a.row_bytes = p->head_dim * es; a.scaling = p->scaling;
    if (pruned > 0) {
        a.k_pruned = k_pruned; a.chan = chan; a.pruned_rows = pruned; a.pruned_dim = x->pruned_dim;
        a.pruned_stride_b = x->pruned_stride_b; a.pruned_stride_h = x->pruned_stride_h;
        a.chan_stride_b = x->chan_stride_b; a.chan_stride_h = x->chan_stride_h;
    }
    a.splits = 1;
    if (workspace) {                                                  // as many splits as the workspace handed over can hold
        const int rows = pruned + p->prefix_rows + p->tail_rows + p->new_rows;
        int s = per_row ? kvc::decode_rows_splits(p->bsz, p->n_q_heads, p->new_rows, rows) : kvc::decode_splits(p->bsz, p->n_q_heads, p->new_rows, rows);
        while (s > 1 && kvc::decode_part_bytes(p->bsz, p->n_q_heads, p->new_rows, p->head_dim, s) > workspace_bytes) --s;
        if (((uintptr_t)workspace) % 16) return fail(KVC_ERR_ALIGNMENT, "workspace is not 16-byte aligned");
        a.splits = s; a.part = static_cast<float*>(workspace);
    }
    if (per_row) {                                                    // kvc_decode_step_rows: p->prefix_rows is the bound of rows_b[]
        kvc::DecodeRowsArgs ra;
        ra.a = a; ra.rows_b = rows_b;
        if (int rc = kvc::launch_decode_step_rows(ra, p->dtype, p->head_dim, static_cast<hipStream_t>(hip_stream)))
            return fail(rc, "no per-row decode kernel for dtype %d head_dim %d", p->dtype, p->head_dim);
        return hip_ok("per-row decode step launch");
    }
    if (int rc = kvc::launch_decode_step(a, p->dtype, p->head_dim, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no decode kernel for dtype %d head_dim %d", p->dtype, p->head_dim);
    return hip_ok("decode step launch");
}
}  // namespace

__attribute__((visibility("default"))) int kvc_decode_step(const kvc_decode_params* p, const void* q, const void* k_new, const void* v_new,
                                                           const void* k_prefix, const void* v_prefix, void* k_tail, void* v_tail,
                                                           void* out, void* hip_stream) {
    return decode_run(p, nullptr, q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, nullptr, nullptr, out, nullptr, 0, hip_stream);
}

__attribute__((visibility("default"))) size_t kvc_decode_workspace_bytes(const kvc_decode_params* p, const kvc_decode_ext* ext) {
    if (decode_check(p, ext)) return 0;
    const int rows = (ext ? ext->pruned_rows : 0) + p->prefix_rows + p->tail_rows + p->new_rows;
    return kvc::decode_part_bytes(p->bsz, p->n_q_heads, p->new_rows, p->head_dim, kvc::decode_splits(p->bsz, p->n_q_heads, p->new_rows, rows));
}

__attribute__((visibility("default"))) int kvc_decode_step2(const kvc_decode_params* p, const kvc_decode_ext* ext, const void* q, const void* k_new,
                                                            const void* v_new, const void* k_prefix, const void* v_prefix, void* k_tail, void* v_tail,
                                                            const void* k_pruned, const int16_t* chan, void* out, void* workspace,
                                                            size_t workspace_bytes, void* hip_stream) {
    return decode_run(p, ext, q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, k_pruned, chan, out, workspace, workspace_bytes, hip_stream);
}

__attribute__((visibility("default"))) size_t kvc_decode_rows_workspace_bytes(const kvc_decode_params* p) {
    if (decode_check(p, nullptr)) return 0;
    const int rows = p->prefix_rows + p->tail_rows + p->new_rows;
    return kvc::decode_part_bytes(p->bsz, p->n_q_heads, p->new_rows, p->head_dim, kvc::decode_rows_splits(p->bsz, p->n_q_heads, p->new_rows, rows));
}

__attribute__((visibility("default"))) int kvc_decode_step_rows(const kvc_decode_params* p, const int32_t* prefix_rows_b, const void* q,
                                                                const void* k_new, const void* v_new, const void* k_prefix, const void* v_prefix,
                                                                void* k_tail, void* v_tail, void* out, void* workspace, size_t workspace_bytes,
                                                                void* hip_stream) {
    return decode_run(p, nullptr, q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, nullptr, nullptr, out, workspace, workspace_bytes,
                      hip_stream, prefix_rows_b, true);
}

// ---- the device-counted decode step (kvc_decode_dev.hip) ------------------------------------------------------------------
namespace {
int decode_dev_check(const kvc_decode_params* p, int32_t tail_capacity) {
    if (!p) return fail(KVC_ERR_INVALID, "params is NULL");
    kvc_decode_params c = *p;
    c.tail_rows = 0;                                                  // ignored here: the device counts
    if (int rc = decode_check(&c, nullptr)) return rc;
    if (tail_capacity < p->new_rows) return fail(KVC_ERR_INVALID, "tail_capacity %d holds fewer rows than the step's new_rows %d", tail_capacity, p->new_rows);
    if ((int64_t)p->prefix_rows + tail_capacity > 0x7fffffffLL) return fail(KVC_ERR_INVALID, "prefix_rows + tail_capacity overflows int32");
    return KVC_OK;
}
}  // namespace

__attribute__((visibility("default"))) size_t kvc_decode_dev_workspace_bytes(const kvc_decode_params* p, int32_t tail_capacity) {
    if (decode_dev_check(p, tail_capacity)) return 0;
    g_err[0] = 0;
    const int rows = p->prefix_rows + tail_capacity;
    return kvc::decode_part_bytes(p->bsz, p->n_q_heads, p->new_rows, p->head_dim, kvc::decode_dev_splits(p->bsz, p->n_q_heads, p->new_rows, rows));
}

namespace {
// kvc_decode_step_dev's checks, every one before any pointer is used, and the kernels' arguments
int decode_dev_args(const kvc_decode_params* p, int32_t tail_capacity, const int32_t* tail_rows_dev, const int32_t* prefix_rows_b,
                    const void* q, const void* k_new, const void* v_new, const void* k_prefix, const void* v_prefix, void* k_tail,
                    void* v_tail, void* out, void* workspace, size_t workspace_bytes, kvc::DecodeDevArgs& da) {
    if (int rc = decode_dev_check(p, tail_capacity)) return rc;
    if (!tail_rows_dev) return fail(KVC_ERR_INVALID, "tail_rows_dev is NULL");
    if (((uintptr_t)tail_rows_dev) % 4) return fail(KVC_ERR_ALIGNMENT, "tail_rows_dev is not 4-byte aligned");
    if (((uintptr_t)prefix_rows_b) % 4) return fail(KVC_ERR_ALIGNMENT, "prefix_rows_b is not 4-byte aligned");
    if (!q || !k_new || !v_new || !k_tail || !v_tail || !out || (p->prefix_rows > 0 && (!k_prefix || !v_prefix)))
        return fail(KVC_ERR_INVALID, "q, k_new, v_new, the tail, out (and the prefix when it has rows) must be non-NULL");
    const int es = esize_of(p->dtype);
    const void* ptrs[] = {q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, out, workspace};
    for (const void* ptr : ptrs) if (((uintptr_t)ptr) % 16) return fail(KVC_ERR_ALIGNMENT, "a pointer is not 16-byte aligned");
    const int64_t strides[] = {p->q_stride_b, p->q_stride_h, p->q_stride_l, p->new_stride_b, p->new_stride_h, p->new_stride_l,
                               p->prefix_stride_b, p->prefix_stride_h, p->tail_stride_b, p->tail_stride_h,
                               p->out_stride_b, p->out_stride_h, p->out_stride_l};
    for (int64_t sd : strides) if ((sd * es) % 16) return fail(KVC_ERR_ALIGNMENT, "a stride is not a multiple of 16 bytes");
    std::memset(&da, 0, sizeof(da));
    kvc::DecodeArgs& a = da.a;
    a.q = q; a.k_new = k_new; a.v_new = v_new; a.k_prefix = k_prefix; a.v_prefix = v_prefix; a.k_tail = k_tail; a.v_tail = v_tail; a.out = out;
    a.q_stride_b = p->q_stride_b; a.q_stride_h = p->q_stride_h; a.q_stride_l = p->q_stride_l;
    a.new_stride_b = p->new_stride_b; a.new_stride_h = p->new_stride_h; a.new_stride_l = p->new_stride_l;
    a.prefix_stride_b = a.vprefix_stride_b = p->prefix_stride_b; a.prefix_stride_h = a.vprefix_stride_h = p->prefix_stride_h;
    a.tail_stride_b = p->tail_stride_b; a.tail_stride_h = p->tail_stride_h;
    a.out_stride_b = p->out_stride_b; a.out_stride_h = p->out_stride_h; a.out_stride_l = p->out_stride_l;
    a.bsz = p->bsz; a.n_q_heads = p->n_q_heads; a.n_kv_heads = p->n_kv_heads; a.group = p->n_q_heads / p->n_kv_heads;
    a.prefix_rows = p->prefix_rows; a.new_rows = p->new_rows;               // p->tail_rows is ignored: the device counts
    a.esize = es; a.row_bytes = p->head_dim * es; a.scaling = p->scaling;
    da.rows_b = prefix_rows_b; da.tail_dev = tail_rows_dev; da.tail_capacity = tail_capacity;
    a.splits = 1;
    if (workspace) {                                                  // as many splits of the BOUND as the workspace can hold
        int s = kvc::decode_dev_splits(p->bsz, p->n_q_heads, p->new_rows, p->prefix_rows + tail_capacity);
        while (s > 1 && kvc::decode_part_bytes(p->bsz, p->n_q_heads, p->new_rows, p->head_dim, s) > workspace_bytes) --s;
        a.splits = s; a.part = static_cast<float*>(workspace);
    }
    return KVC_OK;
}
}  // namespace

__attribute__((visibility("default"))) int kvc_decode_step_dev(const kvc_decode_params* p, int32_t tail_capacity, const int32_t* tail_rows_dev,
                                                               const int32_t* prefix_rows_b, const void* q, const void* k_new, const void* v_new,
                                                               const void* k_prefix, const void* v_prefix, void* k_tail, void* v_tail, void* out,
                                                               void* workspace, size_t workspace_bytes, void* hip_stream) {
    kvc::DecodeDevArgs da;
    if (int rc = decode_dev_args(p, tail_capacity, tail_rows_dev, prefix_rows_b, q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, out,
                                 workspace, workspace_bytes, da)) return rc;
    if (int rc = kvc::launch_decode_step_dev(da, p->dtype, p->head_dim, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no device-counted decode kernel for dtype %d head_dim %d", p->dtype, p->head_dim);
    return hip_ok("device-counted decode step launch");
}

__attribute__((visibility("default"))) int kvc_decode_step_dev_ring(const kvc_decode_params* p, int32_t tail_capacity, const int32_t* tail_rows_dev,
                                                                    const int32_t* prefix_rows_b, const void* q, const void* k_new,
                                                                    const void* v_new, const void* k_prefix, const void* v_prefix, void* k_tail,
                                                                    void* v_tail, void* out, void* q_ring, int32_t ring_rows,
                                                                    int64_t ring_stride_b, int64_t ring_stride_h, void* workspace,
                                                                    size_t workspace_bytes, void* hip_stream) {
    if (int rc = decode_dev_check(p, tail_capacity)) return rc;
    if (ring_rows < 1) return fail(KVC_ERR_INVALID, "ring_rows %d must be >= 1", ring_rows);
    if (!q_ring) return fail(KVC_ERR_INVALID, "q_ring is NULL");
    const int es = esize_of(p->dtype);
    if (((uintptr_t)q_ring) % 16 || (ring_stride_b * es) % 16 || (ring_stride_h * es) % 16)
        return fail(KVC_ERR_INVALID, "q_ring and its strides must be 16-byte aligned");
    if (ring_stride_h < (int64_t)ring_rows * p->head_dim || ring_stride_b < (int64_t)p->n_q_heads * ring_stride_h)
        return fail(KVC_ERR_INVALID, "ring strides (%lld, %lld) smaller than its [heads=%d][rows=%d][head_dim=%d] extent",
                    (long long)ring_stride_b, (long long)ring_stride_h, p->n_q_heads, ring_rows, p->head_dim);
    kvc::DecodeDevRingArgs ra;
    if (int rc = decode_dev_args(p, tail_capacity, tail_rows_dev, prefix_rows_b, q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, out,
                                 workspace, workspace_bytes, ra.d)) return rc;
    ra.ring = q_ring; ra.ring_stride_b = ring_stride_b; ra.ring_stride_h = ring_stride_h; ra.ring_rows = ring_rows;
    if (int rc = kvc::launch_decode_step_dev_ring(ra, p->dtype, p->head_dim, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no device-counted decode kernel for dtype %d head_dim %d", p->dtype, p->head_dim);
    return hip_ok("device-counted decode step (query ring) launch");
}

// ---- quantized decode cache (kvc_quant.hip) -------------------------------------------------------------------------------
namespace {
int quant_common(int dtype, int head_dim, int nbits, int group) {
    if (dtype < KVC_BF16 || dtype > KVC_FP32) return fail(KVC_ERR_INVALID, "unknown dtype %d", dtype);
    if (head_dim != 64 && head_dim != 128) return fail(KVC_ERR_UNSUPPORTED, "quantized cache kernels are built for head_dim 64 and 128, got %d", head_dim);
    if (nbits != 2 && nbits != 4 && nbits != 8) return fail(KVC_ERR_INVALID, "nbits must be 2, 4 or 8, got %d", nbits);
    if (group != 32 && group != 64 && group != 128) return fail(KVC_ERR_UNSUPPORTED, "group_size must be 32, 64 or 128, got %d", group);
    if (head_dim % group) return fail(KVC_ERR_INVALID, "group_size %d does not divide head_dim %d", group, head_dim);
    return KVC_OK;
}
inline int64_t kmeta_floats(int rows, int group, int head_dim) { return (int64_t)((rows + group - 1) / group) * 2 * head_dim; }
inline int64_t vmeta_floats(int rows, int group, int head_dim) { return (int64_t)rows * (head_dim / group) * 2; }

int quant_check(const kvc_quant_params* p) {
    if (!p) return fail(KVC_ERR_INVALID, "params is NULL");
    if (int rc = quant_common(p->dtype, p->head_dim, p->nbits, p->group_size)) return rc;
    if (p->mode != KVC_QUANT_KEYS && p->mode != KVC_QUANT_VALUES) return fail(KVC_ERR_INVALID, "unknown mode %d", p->mode);
    if (p->bsz < 1 || p->n_heads < 1) return fail(KVC_ERR_INVALID, "bsz / n_heads must be positive");
    if (p->rows < 0 || p->row0 < 0 || p->capacity < 0 || (int64_t)p->row0 + p->rows > p->capacity)
        return fail(KVC_ERR_INVALID, "rows [%d, %d + %d) do not fit a capacity of %d", p->row0, p->row0, p->rows, p->capacity);
    if (p->mode == KVC_QUANT_KEYS && p->row0 % p->group_size)
        return fail(KVC_ERR_INVALID, "key rows start at a group boundary: row0 %d is not a multiple of group_size %d", p->row0, p->group_size);
    const int64_t cb = (int64_t)p->head_dim * p->nbits / 8;
    const int64_t mf = p->mode == KVC_QUANT_KEYS ? kmeta_floats(p->capacity, p->group_size, p->head_dim) : vmeta_floats(p->capacity, p->group_size, p->head_dim);
    if (p->code_stride_h < (int64_t)p->capacity * cb || p->code_stride_b < p->n_heads * p->code_stride_h)
        return fail(KVC_ERR_INVALID, "code strides (%lld, %lld) smaller than the %d rows of %lld bytes per head", (long long)p->code_stride_b,
                    (long long)p->code_stride_h, p->capacity, (long long)cb);
    if (p->meta_stride_h < mf || p->meta_stride_b < p->n_heads * p->meta_stride_h)
        return fail(KVC_ERR_INVALID, "metadata strides (%lld, %lld) smaller than the %lld floats per head", (long long)p->meta_stride_b,
                    (long long)p->meta_stride_h, (long long)mf);
    if (p->src_stride_l < p->head_dim || p->src_stride_h < 0 || p->src_stride_b < 0)   // any [b][h][row] order, rows apart
        return fail(KVC_ERR_INVALID, "source / destination strides do not hold rows of head_dim %d", p->head_dim);
    const int ma = p->mode == KVC_QUANT_KEYS ? 4 : 2;              // key metadata is read as float4, value metadata as float2
    if (p->code_stride_b % 16 || p->code_stride_h % 16 || p->meta_stride_b % ma || p->meta_stride_h % ma)
        return fail(KVC_ERR_ALIGNMENT, "code strides must be multiples of 16 bytes and metadata strides of %d floats", ma);
    return KVC_OK;
}
kvc::QuantArgs quant_args(const kvc_quant_params* p) {
    kvc::QuantArgs a;
    std::memset(&a, 0, sizeof(a));
    a.s_stride_b = p->src_stride_b; a.s_stride_h = p->src_stride_h; a.s_stride_l = p->src_stride_l;
    a.c_stride_b = p->code_stride_b; a.c_stride_h = p->code_stride_h; a.m_stride_b = p->meta_stride_b; a.m_stride_h = p->meta_stride_h;
    a.bsz = p->bsz; a.n_heads = p->n_heads; a.head_dim = p->head_dim; a.group = p->group_size; a.row0 = p->row0; a.rows = p->rows;
    return a;
}

int seg_check(const char* what, const kvc_quant_seg* s, int n_heads, int head_dim, int nbits, int group) {
    if (!s) return fail(KVC_ERR_INVALID, "%s segment is NULL", what);
    if (s->rows < 0 || s->capacity < s->rows) return fail(KVC_ERR_INVALID, "%s: %d rows do not fit a capacity of %d", what, s->rows, s->capacity);
    const int64_t cb = (int64_t)head_dim * nbits / 8;
    if (s->code_stride_h < (int64_t)s->capacity * cb || s->code_stride_b < n_heads * s->code_stride_h ||
        s->k_meta_stride_h < kmeta_floats(s->capacity, group, head_dim) || s->k_meta_stride_b < n_heads * s->k_meta_stride_h ||
        s->v_meta_stride_h < vmeta_floats(s->capacity, group, head_dim) || s->v_meta_stride_b < n_heads * s->v_meta_stride_h)
        return fail(KVC_ERR_INVALID, "%s: strides smaller than a capacity of %d rows", what, s->capacity);
    if (s->code_stride_b % 16 || s->code_stride_h % 16 || s->k_meta_stride_b % 4 || s->k_meta_stride_h % 4 ||
        s->v_meta_stride_b % 2 || s->v_meta_stride_h % 2)
        return fail(KVC_ERR_ALIGNMENT, "%s: code strides must be multiples of 16 bytes, key / value metadata strides of 4 / 2 floats", what);
    return KVC_OK;
}
int decode_quant_check(const kvc_decode_quant_params* p, const kvc_quant_seg* pre, const kvc_quant_seg* qt) {
    if (!p) return fail(KVC_ERR_INVALID, "params is NULL");
    if (int rc = quant_common(p->dtype, p->head_dim, p->nbits, p->group_size)) return rc;
    if (p->residual_length < p->group_size || p->residual_length % p->group_size)
        return fail(KVC_ERR_INVALID, "residual_length %d must be a positive multiple of group_size %d", p->residual_length, p->group_size);
    if (p->bsz < 1 || p->n_q_heads < 1 || p->n_kv_heads < 1 || p->n_q_heads % p->n_kv_heads)
        return fail(KVC_ERR_INVALID, "bsz / head counts invalid");
    if (p->new_rows < 1 || p->res_rows < 0 || p->res_rows >= p->residual_length)
        return fail(KVC_ERR_INVALID, "new_rows must be >= 1 and res_rows in [0, residual_length): got %d, %d", p->new_rows, p->res_rows);
    if ((int64_t)p->res_rows + p->new_rows > p->res_capacity)
        return fail(KVC_ERR_INVALID, "%d residual rows + %d new rows do not fit a capacity of %d", p->res_rows, p->new_rows, p->res_capacity);
    if (p->res_stride_h < (int64_t)p->res_capacity * p->head_dim || p->res_stride_b < p->n_kv_heads * p->res_stride_h)
        return fail(KVC_ERR_INVALID, "residual strides smaller than its capacity");
    if (int rc = seg_check("prefix", pre, p->n_q_heads, p->head_dim, p->nbits, p->group_size)) return rc;
    if (int rc = seg_check("quantized tail", qt, p->n_kv_heads, p->head_dim, p->nbits, p->group_size)) return rc;
    if (qt->rows % p->group_size) return fail(KVC_ERR_INVALID, "quantized tail rows %d not a multiple of group_size %d", qt->rows, p->group_size);
    return KVC_OK;
}
int decode_quant_splits(const kvc_decode_quant_params* p, const kvc_quant_seg* pre, const kvc_quant_seg* qt) {
    return kvc::decode_splits(p->bsz, p->n_q_heads, p->new_rows, pre->rows + qt->rows + p->res_rows + p->new_rows);
}
// The launch of kvc_decode_step_quant (o == nullptr) and of kvc_decode_step_quant_outliers: everything but the outlier descriptors.
int decode_quant_run(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix, const kvc_quant_seg* qtail, const kvc::DecodeOArgs* o,
                     const void* q, const void* k_new, const void* v_new, void* k_res, void* v_res, void* out,
                     void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (!q || !k_new || !v_new || !k_res || !v_res || !out)
        return fail(KVC_ERR_INVALID, "q, k_new, v_new, k_res, v_res and out must be non-NULL");
    for (const kvc_quant_seg* s : {prefix, qtail})
        if (s->rows > 0 && (!s->k_codes || !s->v_codes || !s->k_meta || !s->v_meta))
            return fail(KVC_ERR_INVALID, "a segment with rows needs its codes and metadata");
    const int es = esize_of(p->dtype);
    const void* ptrs[] = {q, k_new, v_new, k_res, v_res, out, prefix->k_codes, prefix->v_codes, prefix->k_meta, prefix->v_meta,
                          qtail->k_codes, qtail->v_codes, qtail->k_meta, qtail->v_meta};
    for (const void* ptr : ptrs) if (((uintptr_t)ptr) % 16) return fail(KVC_ERR_ALIGNMENT, "a pointer is not 16-byte aligned");
    const int64_t strides[] = {p->q_stride_b, p->q_stride_h, p->q_stride_l, p->new_stride_b, p->new_stride_h, p->new_stride_l,
                               p->res_stride_b, p->res_stride_h};
    for (int64_t sd : strides) if ((sd * es) % 16) return fail(KVC_ERR_ALIGNMENT, "a stride is not a multiple of 16 bytes");
    kvc::DecodeArgs ap;                                           // append to the residual; combine of the splits
    std::memset(&ap, 0, sizeof(ap));
    ap.k_new = k_new; ap.v_new = v_new; ap.k_tail = k_res; ap.v_tail = v_res; ap.out = out;
    ap.new_stride_b = p->new_stride_b; ap.new_stride_h = p->new_stride_h; ap.new_stride_l = p->new_stride_l;
    ap.tail_stride_b = p->res_stride_b; ap.tail_stride_h = p->res_stride_h;
    ap.out_stride_b = p->out_stride_b; ap.out_stride_h = p->out_stride_h; ap.out_stride_l = p->out_stride_l;
    ap.bsz = p->bsz; ap.n_q_heads = p->n_q_heads; ap.n_kv_heads = p->n_kv_heads; ap.group = p->n_q_heads / p->n_kv_heads;
    ap.tail_rows = p->res_rows; ap.new_rows = p->new_rows; ap.esize = es; ap.row_bytes = p->head_dim * es;
    kvc::DecodeQArgs a;
    std::memset(&a, 0, sizeof(a));
    a.q = q; a.k_res = k_res; a.v_res = v_res; a.out = out;
    a.q_stride_b = p->q_stride_b; a.q_stride_h = p->q_stride_h; a.q_stride_l = p->q_stride_l;
    a.res_stride_b = p->res_stride_b; a.res_stride_h = p->res_stride_h;
    a.out_stride_b = p->out_stride_b; a.out_stride_h = p->out_stride_h; a.out_stride_l = p->out_stride_l;
    kvc::QSegArgs* dst[2] = {&a.pre, &a.qt};
    const kvc_quant_seg* src[2] = {prefix, qtail};
    for (int k = 0; k < 2; ++k) {
        kvc::QSegArgs& d = *dst[k];
        const kvc_quant_seg& s = *src[k];
        d.kc = s.k_codes; d.vc = s.v_codes; d.km = s.k_meta; d.vm = s.v_meta; d.rows = s.rows;
        d.c_stride_b = s.code_stride_b; d.c_stride_h = s.code_stride_h;
        d.km_stride_b = s.k_meta_stride_b; d.km_stride_h = s.k_meta_stride_h; d.vm_stride_b = s.v_meta_stride_b; d.vm_stride_h = s.v_meta_stride_h;
    }
    a.bsz = p->bsz; a.n_q_heads = p->n_q_heads; a.group = p->n_q_heads / p->n_kv_heads; a.gsize = p->group_size;
    a.res_rows = p->res_rows; a.new_rows = p->new_rows; a.scaling = p->scaling;
    a.splits = 1;
    if (workspace) {
        if (((uintptr_t)workspace) % 16) return fail(KVC_ERR_ALIGNMENT, "workspace is not 16-byte aligned");
        int s = decode_quant_splits(p, prefix, qtail);
        while (s > 1 && kvc::decode_part_bytes(p->bsz, p->n_q_heads, p->new_rows, p->head_dim, s) > workspace_bytes) --s;
        a.splits = s; a.part = static_cast<float*>(workspace);
    }
    const int rc = o ? kvc::launch_decode_step_quant_outliers(a, *o, p->dtype, p->head_dim, p->nbits, ap, static_cast<hipStream_t>(hip_stream))
                     : kvc::launch_decode_step_quant(a, p->dtype, p->head_dim, p->nbits, ap, static_cast<hipStream_t>(hip_stream));
    if (rc) return fail(rc, "no quantized decode kernel for dtype %d head_dim %d nbits %d", p->dtype, p->head_dim, p->nbits);
    return hip_ok("quantized decode step launch");
}
}  // namespace

extern "C" {
__attribute__((visibility("default"))) int kvc_quantize_rows(const kvc_quant_params* p, const void* src, uint8_t* codes, float* meta, void* hip_stream) {
    if (int rc = quant_check(p)) return rc;
    if (p->rows == 0) return KVC_OK;
    if (!src || !codes || !meta) return fail(KVC_ERR_INVALID, "src, codes and meta must be non-NULL");
    if (((uintptr_t)codes) % 16 || ((uintptr_t)meta) % 16 || ((uintptr_t)src) % esize_of(p->dtype))
        return fail(KVC_ERR_ALIGNMENT, "codes / meta must be 16-byte aligned, src element-aligned");
    kvc::QuantArgs a = quant_args(p);
    a.src = src; a.codes = codes; a.meta = meta;
    if (int rc = kvc::launch_quantize(a, p->dtype, p->nbits, p->mode, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no quantize kernel for dtype %d nbits %d", p->dtype, p->nbits);
    return hip_ok("quantize launch");
}

__attribute__((visibility("default"))) int kvc_dequantize_rows(const kvc_quant_params* p, const uint8_t* codes, const float* meta, void* dst, void* hip_stream) {
    if (int rc = quant_check(p)) return rc;
    if (p->rows == 0) return KVC_OK;
    if (!dst || !codes || !meta) return fail(KVC_ERR_INVALID, "codes, meta and dst must be non-NULL");
    if (((uintptr_t)codes) % 16 || ((uintptr_t)meta) % 16 || ((uintptr_t)dst) % esize_of(p->dtype))
        return fail(KVC_ERR_ALIGNMENT, "codes / meta must be 16-byte aligned, dst element-aligned");
    kvc::QuantArgs a = quant_args(p);
    a.dst = dst; a.codes_in = codes; a.meta_in = meta;
    if (int rc = kvc::launch_dequantize(a, p->dtype, p->nbits, p->mode, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no de-quantize kernel for dtype %d nbits %d", p->dtype, p->nbits);
    return hip_ok("dequantize launch");
}

__attribute__((visibility("default"))) size_t kvc_decode_quant_workspace_bytes(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix,
                                                                               const kvc_quant_seg* qtail) {
    if (decode_quant_check(p, prefix, qtail)) return 0;
    return kvc::decode_part_bytes(p->bsz, p->n_q_heads, p->new_rows, p->head_dim, decode_quant_splits(p, prefix, qtail));
}

__attribute__((visibility("default"))) int kvc_decode_step_quant(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix, const kvc_quant_seg* qtail,
                                                                 const void* q, const void* k_new, const void* v_new, void* k_res, void* v_res, void* out,
                                                                 void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = decode_quant_check(p, prefix, qtail)) return rc;
    return decode_quant_run(p, prefix, qtail, nullptr, q, k_new, v_new, k_res, v_res, out, workspace, workspace_bytes, hip_stream);
}
}  // extern "C"

// ---- the device-counted quantized decode step (kvc_decode_quant_dev.hip) --------------------------------------------------
namespace {
// kvc_decode_step_quant's checks with the two lengths left to the device, and those of the capacities that bound them
int decode_quant_dev_check(const kvc_decode_quant_params* p, const kvc_quant_seg* pre, const kvc_quant_seg* qt) {
    if (!p) return fail(KVC_ERR_INVALID, "params is NULL");
    if (!qt) return fail(KVC_ERR_INVALID, "quantized tail segment is NULL");
    kvc_decode_quant_params c = *p;
    kvc_quant_seg t = *qt;
    c.res_rows = 0;                                                   // ignored here: the device counts
    t.rows = 0;
    if (p->new_rows >= 1 && p->res_capacity < p->new_rows)
        return fail(KVC_ERR_INVALID, "res_capacity %d holds fewer rows than the step's new_rows %d", p->res_capacity, p->new_rows);
    if (int rc = decode_quant_check(&c, pre, &t)) return rc;
    if (qt->capacity % p->group_size)
        return fail(KVC_ERR_INVALID, "quantized tail capacity %d not a multiple of group_size %d", qt->capacity, p->group_size);
    if ((int64_t)pre->rows + qt->capacity + p->res_capacity > 0x7fffffffLL)
        return fail(KVC_ERR_INVALID, "prefix rows + tail capacity + res_capacity overflows int32");
    return KVC_OK;
}
int decode_quant_dev_splits(const kvc_decode_quant_params* p, const kvc_quant_seg* pre, const kvc_quant_seg* qt) {
    return kvc::decode_splits(p->bsz, p->n_q_heads, p->new_rows, pre->rows + qt->capacity + p->res_capacity);    // the bound
}
}  // namespace

extern "C" {
__attribute__((visibility("default"))) size_t kvc_decode_quant_dev_workspace_bytes(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix,
                                                                                   const kvc_quant_seg* qtail) {
    if (decode_quant_dev_check(p, prefix, qtail)) return 0;
    g_err[0] = 0;
    return kvc::decode_part_bytes(p->bsz, p->n_q_heads, p->new_rows, p->head_dim, decode_quant_dev_splits(p, prefix, qtail));
}

__attribute__((visibility("default"))) int kvc_decode_step_quant_dev(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix,
                                                                     const kvc_quant_seg* qtail, const int32_t* qtail_rows_dev,
                                                                     const int32_t* res_rows_dev, const void* q, const void* k_new,
                                                                     const void* v_new, void* k_res, void* v_res, void* out, void* workspace,
                                                                     size_t workspace_bytes, void* hip_stream) {
    if (int rc = decode_quant_dev_check(p, prefix, qtail)) return rc;
    if (!qtail_rows_dev || !res_rows_dev) return fail(KVC_ERR_INVALID, "qtail_rows_dev / res_rows_dev is NULL");
    if (((uintptr_t)qtail_rows_dev) % 4 || ((uintptr_t)res_rows_dev) % 4)
        return fail(KVC_ERR_ALIGNMENT, "qtail_rows_dev / res_rows_dev is not 4-byte aligned");
    if (!q || !k_new || !v_new || !k_res || !v_res || !out)
        return fail(KVC_ERR_INVALID, "q, k_new, v_new, k_res, v_res and out must be non-NULL");
    if (prefix->rows > 0 && (!prefix->k_codes || !prefix->v_codes || !prefix->k_meta || !prefix->v_meta))
        return fail(KVC_ERR_INVALID, "a prefix with rows needs its codes and metadata");
    if (qtail->capacity > 0 && (!qtail->k_codes || !qtail->v_codes || !qtail->k_meta || !qtail->v_meta))
        return fail(KVC_ERR_INVALID, "a quantized tail with capacity needs its codes and metadata");
    const int es = esize_of(p->dtype);
    const void* ptrs[] = {q, k_new, v_new, k_res, v_res, out, workspace, prefix->k_codes, prefix->v_codes, prefix->k_meta, prefix->v_meta,
                          qtail->k_codes, qtail->v_codes, qtail->k_meta, qtail->v_meta};
    for (const void* ptr : ptrs) if (((uintptr_t)ptr) % 16) return fail(KVC_ERR_ALIGNMENT, "a pointer is not 16-byte aligned");
    const int64_t strides[] = {p->q_stride_b, p->q_stride_h, p->q_stride_l, p->new_stride_b, p->new_stride_h, p->new_stride_l,
                               p->res_stride_b, p->res_stride_h};
    for (int64_t sd : strides) if ((sd * es) % 16) return fail(KVC_ERR_ALIGNMENT, "a stride is not a multiple of 16 bytes");
    kvc::DecodeArgs ap;                                           // the step's rows -> the residual
    std::memset(&ap, 0, sizeof(ap));
    ap.k_new = k_new; ap.v_new = v_new; ap.k_tail = k_res; ap.v_tail = v_res;
    ap.new_stride_b = p->new_stride_b; ap.new_stride_h = p->new_stride_h; ap.new_stride_l = p->new_stride_l;
    ap.tail_stride_b = p->res_stride_b; ap.tail_stride_h = p->res_stride_h;
    ap.bsz = p->bsz; ap.n_q_heads = p->n_q_heads; ap.n_kv_heads = p->n_kv_heads; ap.group = p->n_q_heads / p->n_kv_heads;
    ap.new_rows = p->new_rows; ap.esize = es; ap.row_bytes = p->head_dim * es;
    kvc::DecodeQDevArgs da;
    std::memset(&da, 0, sizeof(da));
    kvc::DecodeQArgs& a = da.a;
    a.q = q; a.k_res = k_res; a.v_res = v_res; a.out = out;
    a.q_stride_b = p->q_stride_b; a.q_stride_h = p->q_stride_h; a.q_stride_l = p->q_stride_l;
    a.res_stride_b = p->res_stride_b; a.res_stride_h = p->res_stride_h;
    a.out_stride_b = p->out_stride_b; a.out_stride_h = p->out_stride_h; a.out_stride_l = p->out_stride_l;
    kvc::QSegArgs* dst[2] = {&a.pre, &a.qt};
    const kvc_quant_seg* src[2] = {prefix, qtail};
    for (int k = 0; k < 2; ++k) {
        kvc::QSegArgs& d = *dst[k];
        const kvc_quant_seg& s = *src[k];
        d.kc = s.k_codes; d.vc = s.v_codes; d.km = s.k_meta; d.vm = s.v_meta; d.rows = k == 0 ? s.rows : 0;    // qtail->rows is ignored
        d.c_stride_b = s.code_stride_b; d.c_stride_h = s.code_stride_h;
        d.km_stride_b = s.k_meta_stride_b; d.km_stride_h = s.k_meta_stride_h; d.vm_stride_b = s.v_meta_stride_b; d.vm_stride_h = s.v_meta_stride_h;
    }
    a.bsz = p->bsz; a.n_q_heads = p->n_q_heads; a.group = p->n_q_heads / p->n_kv_heads; a.gsize = p->group_size;
    a.new_rows = p->new_rows; a.scaling = p->scaling;                 // p->res_rows is ignored: the device counts
    da.qt_dev = qtail_rows_dev; da.res_dev = res_rows_dev; da.qt_capacity = qtail->capacity; da.res_capacity = p->res_capacity;
    a.splits = 1;
    if (workspace) {                                                  // as many splits of the BOUND as the workspace can hold
        int s = decode_quant_dev_splits(p, prefix, qtail);
        while (s > 1 && kvc::decode_part_bytes(p->bsz, p->n_q_heads, p->new_rows, p->head_dim, s) > workspace_bytes) --s;
        a.splits = s; a.part = static_cast<float*>(workspace);
    }
    if (int rc = kvc::launch_decode_step_quant_dev(da, p->dtype, p->head_dim, p->nbits, ap, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no device-counted quantized decode kernel for dtype %d head_dim %d nbits %d", p->dtype, p->head_dim, p->nbits);
    return hip_ok("device-counted quantized decode step launch");
}
}  // extern "C"

// ---- quantized cache with exact outliers (kvc_quant.hip) -----------------------------------------------------------------
namespace {
constexpr int32_t kOutlPoolMax = (1 << 24) - 1;            // rowinfo keeps the first entry in 24 bits

int outl_check(const char* what, const kvc_quant_outliers* o, int bsz, int n_heads, int capacity) {
    if (!o) return fail(KVC_ERR_INVALID, "%s outlier descriptor is NULL", what);
    if (o->pool_capacity < 0 || o->pool_capacity > kOutlPoolMax)
        return fail(KVC_ERR_INVALID, "%s: pool_capacity %d outside [0, %d]", what, o->pool_capacity, kOutlPoolMax);
    if (o->pool_stride_b < o->pool_capacity)
        return fail(KVC_ERR_INVALID, "%s: pool_stride_b %lld smaller than pool_capacity %d", what, (long long)o->pool_stride_b, o->pool_capacity);
    if (o->rowinfo_stride_h < capacity || o->rowinfo_stride_b < (int64_t)n_heads * o->rowinfo_stride_h)
        return fail(KVC_ERR_INVALID, "%s: rowinfo strides (%lld, %lld) smaller than %d rows per head", what, (long long)o->rowinfo_stride_b,
                    (long long)o->rowinfo_stride_h, capacity);
    return KVC_OK;
}
int outl_ptrs(const char* what, const kvc_quant_outliers* o, int dtype) {
    if (!o->used || !o->rowinfo || (o->pool_capacity > 0 && (!o->chan || !o->val)))
        return fail(KVC_ERR_INVALID, "%s: used, rowinfo (and chan, val when pool_capacity > 0) must be non-NULL", what);
    if (((uintptr_t)o->used) % 4 || ((uintptr_t)o->rowinfo) % 4 || ((uintptr_t)o->val) % esize_of(dtype))
        return fail(KVC_ERR_ALIGNMENT, "%s: used / rowinfo must be 4-byte aligned, val element-aligned", what);
    return KVC_OK;
}
int outl_threshold(float threshold, int dtype, float* rounded) {
    if (!(threshold > 0.0f) || !std::isfinite(threshold)) return fail(KVC_ERR_INVALID, "threshold must be finite and > 0, got %g", (double)threshold);
    if (dtype == KVC_BF16) {                                // round to nearest even (finite input: no NaN case)
        uint32_t u;
        std::memcpy(&u, &threshold, 4);
        u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
        std::memcpy(rounded, &u, 4);
    } else if (dtype == KVC_FP16) {
        *rounded = (float)(_Float16)threshold;              // RNE; above the fp16 range: inf (nothing is an outlier then)
    } else {
        *rounded = threshold;
    }
    return KVC_OK;
}
kvc::OutlArgs outl_args(const kvc_quant_outliers* o, float thr) {
    kvc::OutlArgs r;
    std::memset(&r, 0, sizeof(r));
    r.chan = o->chan; r.val = o->val; r.used = o->used; r.rowinfo = o->rowinfo;
    r.pool_stride_b = o->pool_stride_b; r.ri_stride_b = o->rowinfo_stride_b; r.ri_stride_h = o->rowinfo_stride_h;
    r.pool_capacity = o->pool_capacity; r.thr = thr;
    return r;
}
int decode_outl_check(const kvc_decode_quant_params* p, const kvc_quant_seg* pre, const kvc_quant_seg* qt, const kvc_quant_outliers* po,
                      const kvc_quant_outliers* to) {
    if (int rc = decode_quant_check(p, pre, qt)) return rc;
    if (pre->rows > 0) {
        if (!po) return fail(KVC_ERR_INVALID, "prefix outlier descriptors are NULL");
        for (int m = 0; m < 2; ++m) if (int rc = outl_check(m ? "prefix values" : "prefix keys", po + m, p->bsz, p->n_q_heads, pre->capacity)) return rc;
    }
    if (qt->rows > 0) {
        if (!to) return fail(KVC_ERR_INVALID, "quantized tail outlier descriptors are NULL");
        for (int m = 0; m < 2; ++m) if (int rc = outl_check(m ? "tail values" : "tail keys", to + m, p->bsz, p->n_kv_heads, qt->capacity)) return rc;
    }
    return KVC_OK;
}
}  // namespace

extern "C" {
__attribute__((visibility("default"))) int kvc_quantize_rows_outliers(const kvc_quant_params* p, float threshold, const void* src, uint8_t* codes,
                                                                      float* meta, const kvc_quant_outliers* outl, void* hip_stream) {
    if (int rc = quant_check(p)) return rc;
    float thr = 0.0f;
    if (int rc = outl_threshold(threshold, p->dtype, &thr)) return rc;
    if (int rc = outl_check("outliers", outl, p->bsz, p->n_heads, p->capacity)) return rc;
    if (p->rows == 0) return KVC_OK;
    if (!src || !codes || !meta) return fail(KVC_ERR_INVALID, "src, codes and meta must be non-NULL");
    if (int rc = outl_ptrs("outliers", outl, p->dtype)) return rc;
    if (((uintptr_t)codes) % 16 || ((uintptr_t)meta) % 16 || ((uintptr_t)src) % esize_of(p->dtype))
        return fail(KVC_ERR_ALIGNMENT, "codes / meta must be 16-byte aligned, src element-aligned");
    kvc::QuantArgs a = quant_args(p);
    a.src = src; a.codes = codes; a.meta = meta;
    if (int rc = kvc::launch_quantize_outliers(a, outl_args(outl, thr), p->dtype, p->nbits, p->mode, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no quantize kernel for dtype %d nbits %d", p->dtype, p->nbits);
    return hip_ok("quantize (outliers) launch");
}

__attribute__((visibility("default"))) int kvc_dequantize_rows_outliers(const kvc_quant_params* p, const uint8_t* codes, const float* meta,
                                                                        const kvc_quant_outliers* outl, void* dst, void* hip_stream) {
    if (int rc = quant_check(p)) return rc;
    if (int rc = outl_check("outliers", outl, p->bsz, p->n_heads, p->capacity)) return rc;
    if (p->rows == 0) return KVC_OK;
    if (!dst || !codes || !meta) return fail(KVC_ERR_INVALID, "codes, meta and dst must be non-NULL");
    if (int rc = outl_ptrs("outliers", outl, p->dtype)) return rc;
    if (((uintptr_t)codes) % 16 || ((uintptr_t)meta) % 16 || ((uintptr_t)dst) % esize_of(p->dtype))
        return fail(KVC_ERR_ALIGNMENT, "codes / meta must be 16-byte aligned, dst element-aligned");
    kvc::QuantArgs a = quant_args(p);
    a.dst = dst; a.codes_in = codes; a.meta_in = meta;
    if (int rc = kvc::launch_dequantize_outliers(a, outl_args(outl, 0.0f), p->dtype, p->nbits, p->mode, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no de-quantize kernel for dtype %d nbits %d", p->dtype, p->nbits);
    return hip_ok("dequantize (outliers) launch");
}

__attribute__((visibility("default"))) size_t kvc_decode_quant_outliers_workspace_bytes(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix,
                                                                                        const kvc_quant_seg* qtail, const kvc_quant_outliers* prefix_outl,
                                                                                        const kvc_quant_outliers* qtail_outl) {
    if (decode_outl_check(p, prefix, qtail, prefix_outl, qtail_outl)) return 0;
    return kvc_decode_quant_workspace_bytes(p, prefix, qtail);
}

__attribute__((visibility("default"))) int kvc_decode_step_quant_outliers(const kvc_decode_quant_params* p, const kvc_quant_seg* prefix,
                                                                          const kvc_quant_seg* qtail, const kvc_quant_outliers* prefix_outl,
                                                                          const kvc_quant_outliers* qtail_outl, const void* q, const void* k_new,
                                                                          const void* v_new, void* k_res, void* v_res, void* out, void* workspace,
                                                                          size_t workspace_bytes, void* hip_stream) {
    if (int rc = decode_outl_check(p, prefix, qtail, prefix_outl, qtail_outl)) return rc;
    kvc::DecodeOArgs o;
    std::memset(&o, 0, sizeof(o));
    const kvc_quant_seg* segs[2] = {prefix, qtail};
    const kvc_quant_outliers* outs[2] = {prefix_outl, qtail_outl};
    kvc::OSegArgs* dsts[2] = {&o.pre, &o.qt};
    for (int k = 0; k < 2; ++k) {
        if (segs[k]->rows == 0) continue;
        const kvc_quant_outliers* ko = outs[k];
        const kvc_quant_outliers* vo = outs[k] + 1;
        for (const kvc_quant_outliers* x : {ko, vo})
            if (int rc = outl_ptrs(k ? "tail outliers" : "prefix outliers", x, p->dtype)) return rc;
        kvc::OSegArgs& d = *dsts[k];
        d.kch = ko->chan; d.vch = vo->chan; d.kval = ko->val; d.vval = vo->val; d.kri = ko->rowinfo; d.vri = vo->rowinfo;
        d.kpool_b = ko->pool_stride_b; d.vpool_b = vo->pool_stride_b;
        d.kri_b = ko->rowinfo_stride_b; d.kri_h = ko->rowinfo_stride_h; d.vri_b = vo->rowinfo_stride_b; d.vri_h = vo->rowinfo_stride_h;
        d.kcap = ko->pool_capacity; d.vcap = vo->pool_capacity;
    }
    return decode_quant_run(p, prefix, qtail, &o, q, k_new, v_new, k_res, v_res, out, workspace, workspace_bytes, hip_stream);
}
}  // extern "C"

// ---- AdaKV / HeadKV -------------------------------------------------------------------------------------------------------
namespace {
struct RaggedLayout { size_t ratio, idx, sort, flat, top, sel, total; };
RaggedLayout ragged_carve(const kvc_params* p, const Layout& l) {
    RaggedLayout r;
    const size_t heads = (size_t)p->bsz * p->n_q_heads, n = (size_t)(p->q_len - p->window);
    size_t off = l.total;
    r.ratio = off; off = align_up(off + heads * 4, 256);
    r.idx = off;   off = align_up(off + heads * n * 8, 256);
    r.sort = off;  off = align_up(off + kvc::sort_prefix_scratch_bytes((int)heads, (int)n), 256);
    r.flat = r.top = r.sel = off;
    if (p->method == KVC_ADAKV && p->tie_mode == KVC_TIES_TORCH_CPU) {        // the reference's own flattened top-(H*base)
        const size_t n_tot = (size_t)p->n_q_heads * n, k_tot = (size_t)p->n_q_heads * (size_t)p->k;
        r.flat = off; off = align_up(off + (size_t)p->bsz * n_tot * esize_of(p->dtype), 256);
        r.top = off;  off = align_up(off + (size_t)p->bsz * k_tot * 8, 256);
        r.sel = off;  off = align_up(off + kvc::select_exact_scratch_bytes(p->bsz, (int)n_tot, (int)k_tot), 256);
    }
    r.total = off;
    return r;
}
int ragged_check(const kvc_params* p) {
    if (int rc = validate(p, true)) return rc;
    if (!ragged(p->method)) return fail(KVC_ERR_INVALID, "kvc_ragged_*: method must be KVC_ADAKV or KVC_HEADKV");
    if (p->n_q_heads > 256) return fail(KVC_ERR_UNSUPPORTED, "more than 256 heads");
    return KVC_OK;
}
}  // namespace

__attribute__((visibility("default"))) size_t kvc_ragged_workspace_bytes(const kvc_params* p) {
    if (ragged_check(p) != KVC_OK) return 0;
    g_err[0] = 0;
    kvc_params pk = *p;
    pk.k = 0;
    return ragged_carve(p, carve(&pk)).total;
}

__attribute__((visibility("default"))) int kvc_ragged_plan(const kvc_params* p, const void* q, const void* k, float floor_ratio,
                                                           int normalize, int32_t* caps_out, int32_t* flags_out, void* scores_out,
                                                           void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = ragged_check(p)) return rc;
    if (!q || !k) return fail(KVC_ERR_INVALID, "q and k must be non-NULL");
    const int es = esize_of(p->dtype);
    if (int rc = check_strides("q", es, p->q_stride_b, p->q_stride_h, p->q_stride_l, q)) return rc;
    if (int rc = check_strides("k", es, p->k_stride_b, p->k_stride_h, p->k_stride_l, k)) return rc;
    kvc_params pk = *p;
    pk.k = 0;
    const Layout l = carve(&pk);
    const RaggedLayout r = ragged_carve(p, l);
    if (!workspace || ((uintptr_t)workspace) % 256 || workspace_bytes < r.total)
        return fail(KVC_ERR_WORKSPACE, "kvc_ragged_plan needs %zu bytes of 256-byte aligned workspace", r.total);
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Items it;
    std::memset(&it, 0, sizeof(it));
    it.n = 1; it.q[0] = q; it.k[0] = k; it.scores[0] = ws + l.scores;
    if (int rc = enqueue_scores(&pk, l, it, ws, st)) return rc;
    const size_t heads = (size_t)p->bsz * p->n_q_heads, n = (size_t)(p->q_len - p->window);
    if (scores_out) {
        if (hipMemcpyAsync(scores_out, ws + l.scores, heads * n * es, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return fail(KVC_ERR_HIP, "copy of the scores failed");
    }
    if (p->method == KVC_ADAKV) {
        if (!caps_out) return fail(KVC_ERR_INVALID, "caps_out must be non-NULL for AdaKV");
        if (p->k < 1 || (size_t)p->k > n) return fail(KVC_ERR_INVALID, "base capacity k=%d outside [1, q_len - window]", p->k);
        if (!(floor_ratio >= 0.0f && floor_ratio <= 1.0f)) return fail(KVC_ERR_INVALID, "floor_ratio outside [0, 1]");
        kvc::RaggedArgs a;
        std::memset(&a, 0, sizeof(a));
        a.scores = ws + l.scores;
        a.ratio = reinterpret_cast<float*>(ws + r.ratio);
        a.caps = caps_out;
        a.flags = flags_out ? flags_out : reinterpret_cast<int32_t*>(ws + r.sort);     // (scratch slot when not wanted)
        a.n = (int)n; a.heads_per_batch = p->n_q_heads; a.base = p->k; a.normalize = normalize ? 1 : 0;
        a.floor_capacity = (int)((double)p->k * (double)floor_ratio);                 // int(base_capacity * floor_ratio), :632
        a.mix = (float)(1.0 - (double)floor_ratio);
        if (p->tie_mode == KVC_TIES_TORCH_CPU) {
            // exactly the reference: every head's whole descending sort, the normalised values in that order, torch-CPU's
            // top-(H*base) over the flattened array (libstdc++ partial_sort / nth_element: one wave walks it), counts per head
            const int64_t n_tot = (int64_t)p->n_q_heads * (int64_t)n, k_tot = (int64_t)p->n_q_heads * p->k;
            if (n_tot > 0x7fffffff) return fail(KVC_ERR_UNSUPPORTED, "flattened score array too long");
            kvc::RaggedSortArgs sa;
            sa.scores = ws + l.scores; sa.caps = nullptr; sa.idx_out = reinterpret_cast<int64_t*>(ws + r.idx);
            sa.n = (int)n; sa.heads = (int)heads; sa.out_stride = (int)n;
            if (int rc = kvc::launch_sort_prefix(sa, p->dtype, ws + r.sort, st)) return fail(rc, "sort launch failed");
            if (a.normalize) kvc::launch_ragged_head_stats(a, p->dtype, p->bsz, st);
            kvc::launch_ragged_flatten(a, p->dtype, p->bsz, sa.idx_out, ws + r.flat, st);
            kvc_params ps = *p;
            ps.bsz = p->bsz; ps.n_q_heads = 1; ps.n_kv_heads = 1; ps.q_len = (int)n_tot + p->window; ps.k = (int)k_tot;
            Items sel;
            std::memset(&sel, 0, sizeof(sel));
            sel.n = 1; sel.scores[0] = ws + r.flat; sel.idx[0] = reinterpret_cast<int64_t*>(ws + r.top); sel.keep[0] = (int)k_tot; sel.k_max = (int)k_tot;
            // (only WHICH elements torch's top-(H*base) holds matters here, not their order: the final __sort_heap — a fifth of the
            // walk — is skipped)
            if (int rc = enqueue_select(&ps, sel, false, ws + r.sel, st, true)) return rc;
            kvc::launch_ragged_recount(a, p->bsz, reinterpret_cast<const int64_t*>(ws + r.top), st);
        } else if (int rc = kvc::launch_ragged_plan(a, p->dtype, p->bsz, st)) {
            return fail(rc, "ragged plan launch failed");
        }
    }
    return hip_ok("ragged plan launch");
}

__attribute__((visibility("default"))) int kvc_ragged_compact(const kvc_params* p, const void* k, const void* v, const int32_t* caps,
                                                              const int64_t* seg_off, int rows_max, void* k_flat, void* v_flat,
                                                              int64_t* idx_out, int64_t idx_stride, void* workspace,
                                                              size_t workspace_bytes, void* hip_stream) {
    if (int rc = ragged_check(p)) return rc;
    if (!k || !v || !caps || !seg_off || !k_flat || !v_flat) return fail(KVC_ERR_INVALID, "k, v, caps, seg_off and the flat buffers must be non-NULL");
    const int es = esize_of(p->dtype);
    if (int rc = check_strides("k", es, p->k_stride_b, p->k_stride_h, p->k_stride_l, k)) return rc;
    if (int rc = check_strides("v", es, p->v_stride_b, p->v_stride_h, p->v_stride_l, v)) return rc;
    if (((uintptr_t)k_flat) % 16 || ((uintptr_t)v_flat) % 16) return fail(KVC_ERR_ALIGNMENT, "flat buffers not 16-byte aligned");
    kvc_params pk = *p;
    pk.k = 0;
    const Layout l = carve(&pk);
    const RaggedLayout r = ragged_carve(p, l);
    if (!workspace || ((uintptr_t)workspace) % 256 || workspace_bytes < r.total)
        return fail(KVC_ERR_WORKSPACE, "kvc_ragged_compact needs %zu bytes of 256-byte aligned workspace", r.total);
    const int heads = p->bsz * p->n_q_heads, n = p->q_len - p->window;
    if (rows_max < p->window || rows_max > n + p->window) return fail(KVC_ERR_INVALID, "rows_max %d outside [window, q_len]", rows_max);
    if (idx_out && idx_stride < rows_max - p->window) return fail(KVC_ERR_INVALID, "idx_stride smaller than the largest capacity");
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    kvc::RaggedSortArgs sa;
    sa.scores = ws + l.scores; sa.caps = caps;
    sa.idx_out = idx_out ? idx_out : reinterpret_cast<int64_t*>(ws + r.idx);
    sa.n = n; sa.heads = heads; sa.out_stride = idx_out ? (int)idx_stride : n;
    // (AdaKV with torch_cpu ties: kvc_ragged_plan left every head's whole sort in the workspace — its prefix is the answer)
    const bool presorted = p->method == KVC_ADAKV && p->tie_mode == KVC_TIES_TORCH_CPU && !idx_out;
    if (!presorted)
        if (int rc = kvc::launch_sort_prefix(sa, p->dtype, ws + r.sort, st)) return fail(rc, "sort prefix launch failed");
    kvc::RaggedGatherArgs g;
    std::memset(&g, 0, sizeof(g));
    g.k = k; g.v = v; g.k_flat = k_flat; g.v_flat = v_flat;
    g.idx = sa.idx_out; g.idx_stride = sa.out_stride; g.caps = caps; g.seg_off = seg_off;
    g.k_stride_b = p->k_stride_b; g.k_stride_h = p->k_stride_h; g.k_stride_l = p->k_stride_l;
    g.v_stride_b = p->v_stride_b; g.v_stride_h = p->v_stride_h; g.v_stride_l = p->v_stride_l;
    g.n_q_heads = p->n_q_heads; g.group = p->n_q_heads / p->n_kv_heads; g.q_len = p->q_len; g.window = p->window;
    g.esize = es; g.row_bytes = p->head_dim * es;
    kvc::launch_ragged_gather(g, rows_max, heads, st);
    return hip_ok("ragged compact launch");
}

// ---- L2NormCluster.update_kv (pyramidkv_utils.py:394-429) ---------------------------------------------
namespace {
struct L2Layout { size_t norms, idx, sort, total; };
L2Layout l2norm_carve(const kvc_params* p) {
    L2Layout l;
    const size_t heads = (size_t)p->bsz * p->n_q_heads, L = (size_t)p->q_len;
    size_t off = 0;
    l.norms = off; off = align_up(off + heads * L * esize_of(p->dtype), 256);
    l.idx = off;   off = align_up(off + heads * (size_t)p->k * 8, 256);
    l.sort = off;  off = align_up(off + kvc::sort_prefix_scratch_bytes((int)heads, (int)L), 256);
    l.total = off;
    return l;
}
int l2norm_check(const kvc_params* p) {
    if (!p) return fail(KVC_ERR_INVALID, "params is NULL");
    if (p->method != KVC_L2NORM) return fail(KVC_ERR_INVALID, "kvc_l2norm_*: method must be KVC_L2NORM");
    if (p->dtype < KVC_BF16 || p->dtype > KVC_FP32) return fail(KVC_ERR_INVALID, "unknown dtype %d", p->dtype);
    if (p->bsz < 1 || p->n_q_heads < 1 || p->n_kv_heads < 1) return fail(KVC_ERR_INVALID, "bsz / head counts must be positive");
    if (p->n_q_heads % p->n_kv_heads) return fail(KVC_ERR_INVALID, "n_q_heads %d not a multiple of n_kv_heads %d", p->n_q_heads, p->n_kv_heads);
    if (p->q_len < 1) return fail(KVC_ERR_INVALID, "q_len must be positive");
    if (p->k < 1 || p->k > p->q_len) return fail(KVC_ERR_INVALID, "k=%d outside [1, q_len=%d] (rows kept = max_capacity_prompt)", p->k, p->q_len);
    const int es = esize_of(p->dtype);
    if (p->head_dim < 1 || (p->head_dim * es) % 32) return fail(KVC_ERR_UNSUPPORTED, "head_dim*esize must be a multiple of 32 bytes");
    if (p->head_dim * es > 4096) return fail(KVC_ERR_UNSUPPORTED, "head_dim too large");
    return KVC_OK;
}
}  // namespace

__attribute__((visibility("default"))) size_t kvc_l2norm_workspace_bytes(const kvc_params* p) {
    if (l2norm_check(p) != KVC_OK) return 0;
    g_err[0] = 0;
    return l2norm_carve(p).total;
}

__attribute__((visibility("default"))) int kvc_l2norm_compress(const kvc_params* p, const void* k, const void* v, void* k_out, void* v_out,
                                                               int64_t* idx_out, void* norms_out, void* workspace, size_t workspace_bytes,
                                                               void* hip_stream) {
    if (int rc = l2norm_check(p)) return rc;
    if (!k || !v || !k_out || !v_out) return fail(KVC_ERR_INVALID, "k, v, k_out and v_out must be non-NULL");
    const int es = esize_of(p->dtype);
    if (int rc = check_strides("k", es, p->k_stride_b, p->k_stride_h, p->k_stride_l, k)) return rc;
    if (int rc = check_strides("v", es, p->v_stride_b, p->v_stride_h, p->v_stride_l, v)) return rc;
    if (((uintptr_t)k_out) % 16 || ((uintptr_t)v_out) % 16) return fail(KVC_ERR_ALIGNMENT, "outputs not 16-byte aligned");
    if (p->out_stride_h && (p->out_stride_h < (int64_t)p->k * p->head_dim || (p->out_stride_h * es) % 16))
        return fail(KVC_ERR_INVALID, "out_stride_h smaller than k * head_dim, or not a multiple of 16 bytes");
    const L2Layout l = l2norm_carve(p);
    if (!workspace || ((uintptr_t)workspace) % 256 || workspace_bytes < l.total)
        return fail(KVC_ERR_WORKSPACE, "kvc_l2norm_compress needs %zu bytes of 256-byte aligned workspace", l.total);
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int heads = p->bsz * p->n_q_heads;
    kvc::L2NormArgs na;
    na.k = k; na.norms = norms_out ? norms_out : ws + l.norms;
    na.stride_b = p->k_stride_b; na.stride_h = p->k_stride_h; na.stride_l = p->k_stride_l;
    na.bsz = p->bsz; na.n_q_heads = p->n_q_heads; na.n_kv_heads = p->n_kv_heads; na.q_len = p->q_len; na.head_dim = p->head_dim;
    if (int rc = kvc::launch_l2norm(na, p->dtype, st)) return fail(rc, "l2norm launch failed");
    kvc::RaggedSortArgs sa;
    sa.scores = na.norms; sa.caps = nullptr;
    sa.idx_out = idx_out ? idx_out : reinterpret_cast<int64_t*>(ws + l.idx);
    sa.n = p->q_len; sa.heads = heads; sa.out_stride = p->k; sa.want_fixed = p->k; sa.ascending = 1;
    if (int rc = kvc::launch_sort_prefix(sa, p->dtype, ws + l.sort, st)) return fail(rc, "sort prefix launch failed");
    kvc::GatherArgs g[2];
    for (int which = 0; which < 2; ++which) {
        std::memset(&g[which], 0, sizeof(g[which]));
        g[which].src.p[0] = which ? v : k;
        g[which].out.p[0] = which ? v_out : k_out;
        g[which].idx.p[0] = sa.idx_out;
        g[which].k.v[0] = p->k;
        g[which].out_head_bytes.v[0] = p->out_stride_h * es;
        g[which].n_items = 1; g[which].k_max = p->k;
        g[which].stride_b = which ? p->v_stride_b : p->k_stride_b;
        g[which].stride_h = which ? p->v_stride_h : p->k_stride_h;
        g[which].stride_l = which ? p->v_stride_l : p->k_stride_l;
        g[which].bsz = p->bsz; g[which].n_q_heads = p->n_q_heads; g[which].group = p->n_q_heads / p->n_kv_heads;
        g[which].q_len = p->q_len; g[which].window = 0;
        g[which].esize = es; g[which].row_bytes = p->head_dim * es;
    }
    return enqueue_gather(&g[0], &g[1], st);
}

// ---- merge_kv(..., "pivot") (pyramidkv_utils.py:119-170) ----------------------------------------------------
namespace {
struct MergeLayout { size_t mask, drop, drop_len, kn, pivot, total; };
MergeLayout merge_carve(const kvc_params* p) {
    MergeLayout l;
    const size_t heads = (size_t)p->bsz * p->n_q_heads, L = (size_t)p->q_len, R = (size_t)p->k + p->window;
    size_t off = 0;
    l.mask = off;     off = align_up(off + (size_t)p->bsz * L * 4, 256);
    l.drop = off;     off = align_up(off + (size_t)p->bsz * L * 4, 256);
    l.drop_len = off; off = align_up(off + (size_t)p->bsz * 4, 256);
    l.kn = off;       off = align_up(off + heads * R * 128 * 4, 256);
    l.pivot = off;    off = align_up(off + heads * L * 4, 256);
    l.total = off;
    return l;
}
int merge_check(const kvc_params* p) {
    if (int rc = validate(p, false)) return rc;
    if (p->method != KVC_SNAPKV && p->method != KVC_PYRAMIDKV && p->method != KVC_H2O && p->method != KVC_STREAMINGLLM)
        return fail(KVC_ERR_INVALID, "kvc_merge_pivot: merge_kv is reached from SnapKV / PyramidKV / H2O / StreamingLLM update_kv only");
    if (p->head_dim != 128) return fail(KVC_ERR_UNSUPPORTED, "merge_kv hard-codes head_dim 128 (pyramidkv_utils.py:149), got %d", p->head_dim);
    if (p->dtype == KVC_FP32) return fail(KVC_ERR_UNSUPPORTED, "merge_kv: fp32 not built (torch's fp32 GEMM order is not restated)");
    if (p->k < 1) return fail(KVC_ERR_INVALID, "merge_kv needs k >= 1");
    return KVC_OK;
}
}  // namespace

__attribute__((visibility("default"))) size_t kvc_merge_workspace_bytes(const kvc_params* p) {
    if (merge_check(p) != KVC_OK) return 0;
    g_err[0] = 0;
    return merge_carve(p).total;
}

__attribute__((visibility("default"))) int kvc_merge_pivot(const kvc_params* p, const void* k, const void* v, const int64_t* idx,
                                                           void* k_out, void* v_out, int32_t* pivot_out, int32_t* drop_len_out,
                                                           void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = merge_check(p)) return rc;
    if (!k || !v || !idx || !k_out || !v_out) return fail(KVC_ERR_INVALID, "k, v, idx, k_out and v_out must be non-NULL");
    const int es = esize_of(p->dtype);
    if (int rc = check_strides("k", es, p->k_stride_b, p->k_stride_h, p->k_stride_l, k)) return rc;
    if (int rc = check_strides("v", es, p->v_stride_b, p->v_stride_h, p->v_stride_l, v)) return rc;
    if (((uintptr_t)k_out) % 16 || ((uintptr_t)v_out) % 16) return fail(KVC_ERR_ALIGNMENT, "outputs not 16-byte aligned");
    const int64_t rows = (int64_t)p->k + p->window;
    if (p->out_stride_h && (p->out_stride_h < rows * p->head_dim || (p->out_stride_h * es) % 16))
        return fail(KVC_ERR_INVALID, "out_stride_h smaller than (k + window) * head_dim, or not a multiple of 16 bytes");
    const MergeLayout l = merge_carve(p);
    if (!workspace || ((uintptr_t)workspace) % 256 || workspace_bytes < l.total)
        return fail(KVC_ERR_WORKSPACE, "kvc_merge_pivot needs %zu bytes of 256-byte aligned workspace", l.total);
    char* ws = static_cast<char*>(workspace);
    kvc::MergeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.k = k; a.v = v; a.idx = idx; a.k_out = k_out; a.v_out = v_out;
    a.mask = reinterpret_cast<int32_t*>(ws + l.mask);
    a.drop = reinterpret_cast<int32_t*>(ws + l.drop);
    a.drop_len = drop_len_out ? drop_len_out : reinterpret_cast<int32_t*>(ws + l.drop_len);
    a.kn = reinterpret_cast<float*>(ws + l.kn);
    a.pivot = pivot_out ? pivot_out : reinterpret_cast<int32_t*>(ws + l.pivot);
    a.k_stride_b = p->k_stride_b; a.k_stride_h = p->k_stride_h; a.k_stride_l = p->k_stride_l;
    a.v_stride_b = p->v_stride_b; a.v_stride_h = p->v_stride_h; a.v_stride_l = p->v_stride_l;
    a.out_stride_h = p->out_stride_h;
    a.bsz = p->bsz; a.n_q_heads = p->n_q_heads; a.group = p->n_q_heads / p->n_kv_heads; a.q_len = p->q_len;
    a.window = p->window; a.n_keep = p->k; a.rows = (int)rows;
    if (int rc = kvc::launch_merge(a, p->dtype, static_cast<hipStream_t>(hip_stream))) return fail(rc, "merge launch failed");
    return hip_ok("merge launch");
}

// ---- ThinK channel pruning (pyramidkv_utils.py:13-26) -------------------------------------------------------
__attribute__((visibility("default"))) int kvc_think_prune(const kvc_think_params* p, const void* q, const void* kc, void* pruned,
                                                           uint8_t* keep, void* channel_scores, void* hip_stream) {
    if (!p || !q || !kc || !keep) return fail(KVC_ERR_INVALID, "params, q, kc and keep must be non-NULL");
    if (!pruned && p->rows > p->recent) return fail(KVC_ERR_INVALID, "pruned must be non-NULL");
    if (p->dtype < KVC_BF16 || p->dtype > KVC_FP32) return fail(KVC_ERR_INVALID, "unknown dtype %d", p->dtype);
    if (p->bsz < 1 || p->n_heads < 1) return fail(KVC_ERR_INVALID, "bsz / n_heads must be positive");
    if (p->head_dim != 64 && p->head_dim != 128) return fail(KVC_ERR_UNSUPPORTED, "ThinK pruning is built for head_dim 64 and 128, got %d", p->head_dim);
    if (p->q_len < 32) return fail(KVC_ERR_INVALID, "q_len %d < 32 (the reference reads the last 32 query rows, :17)", p->q_len);
    if (p->rows < 1 || p->recent < 0 || p->recent > p->rows) return fail(KVC_ERR_INVALID, "recent=%d outside [0, rows=%d]", p->recent, p->rows);
    if (p->n_prune < 0 || p->n_prune > p->head_dim) return fail(KVC_ERR_INVALID, "n_prune=%d outside [0, head_dim]", p->n_prune);
    if (p->kc_stride_h < (int64_t)p->rows * p->head_dim) return fail(KVC_ERR_INVALID, "kc_stride_h smaller than rows * head_dim");
    kvc::ThinkArgs a;
    std::memset(&a, 0, sizeof(a));
    a.q = q; a.kc = kc; a.pruned = pruned; a.keep = keep; a.scores = channel_scores;
    a.q_stride_b = p->q_stride_b; a.q_stride_h = p->q_stride_h; a.q_stride_l = p->q_stride_l; a.kc_stride_h = p->kc_stride_h;
    a.bsz = p->bsz; a.n_heads = p->n_heads; a.q_len = p->q_len; a.head_dim = p->head_dim;
    a.rows = p->rows; a.recent = p->recent; a.n_prune = p->n_prune;
    if (int rc = kvc::launch_think(a, p->dtype, static_cast<hipStream_t>(hip_stream))) return fail(rc, "think launch failed");
    return hip_ok("think launch");
}

// ---- CAM (pyramidkv_utils.py:431-513), split at its random draw --------------------------------------------
namespace {
int cam_check(const kvc_params* p, int start_budget) {
    if (int rc = validate(p, true)) return rc;
    if (p->method != KVC_SNAPKV || p->pooling != KVC_POOL_NONE)
        return fail(KVC_ERR_INVALID, "kvc_cam_*: method must be KVC_SNAPKV with KVC_POOL_NONE (CAM scores without pooling, :468-476)");
    if (start_budget < 1 || start_budget + p->window >= p->q_len)
        return fail(KVC_ERR_INVALID, "start_budget %d: the merge loop needs 1 <= start_budget and start_budget + window < q_len", start_budget);
    return KVC_OK;
}
size_t cam_colmean_off(const Layout& l) { return align_up(l.total, 256); }
}  // namespace

__attribute__((visibility("default"))) size_t kvc_cam_workspace_bytes(const kvc_params* p) {
    if (validate(p, true)) return 0;
    const Layout l = carve(p);
    return cam_colmean_off(l) + align_up((size_t)p->bsz * p->n_q_heads * p->q_len * esize_of(p->dtype), 256);
}

__attribute__((visibility("default"))) int kvc_cam_plan(const kvc_params* p, const void* q, const void* k, int start_budget, void* scores_out,
                                                        void* prob_out, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = cam_check(p, start_budget)) return rc;
    if (!q || !k || !scores_out || !prob_out) return fail(KVC_ERR_INVALID, "q, k, scores_out and prob_out must be non-NULL");
    const int es = esize_of(p->dtype);
    if (int rc = check_strides("q", es, p->q_stride_b, p->q_stride_h, p->q_stride_l, q)) return rc;
    if (int rc = check_strides("k", es, p->k_stride_b, p->k_stride_h, p->k_stride_l, k)) return rc;
    const Layout l = carve(p);
    if (!workspace || ((uintptr_t)workspace) % 256 || workspace_bytes < kvc_cam_workspace_bytes(p))
        return fail(KVC_ERR_WORKSPACE, "workspace NULL, misaligned or smaller than kvc_cam_workspace_bytes");
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Items it;
    std::memset(&it, 0, sizeof(it));
    it.n = 1; it.q[0] = q; it.k[0] = k; it.scores[0] = scores_out;
    if (int rc = enqueue_scores(p, l, it, ws, st)) return rc;            // window-row sums, no pooling: the reference's attn_cache
    kvc::CamArgs a;
    std::memset(&a, 0, sizeof(a));
    a.logits = ws + l.logits; a.rowmax = reinterpret_cast<const float*>(ws + l.rowmax); a.rowsum = reinterpret_cast<const float*>(ws + l.rowsum);
    a.colmean = ws + cam_colmean_off(l); a.prob = prob_out;
    a.bsz = p->bsz; a.n_q_heads = p->n_q_heads; a.q_len = p->q_len; a.window = p->window; a.start = start_budget;
    if (int rc = kvc::launch_cam_prob(a, p->dtype, st)) return fail(rc, "no CAM kernel for dtype %d", p->dtype);
    return hip_ok("cam plan launch");
}

__attribute__((visibility("default"))) int kvc_cam_merge(const kvc_params* p, void* v, const uint8_t* merge_mask, int start_budget, void* hip_stream) {
    if (int rc = cam_check(p, start_budget)) return rc;
    if (!v || !merge_mask) return fail(KVC_ERR_INVALID, "v and merge_mask must be non-NULL");
    if (p->head_dim > 256) return fail(KVC_ERR_UNSUPPORTED, "head_dim > 256");
    kvc::CamArgs a;
    std::memset(&a, 0, sizeof(a));
    a.v = v; a.mask = merge_mask;
    a.v_stride_b = p->v_stride_b; a.v_stride_h = p->v_stride_h; a.v_stride_l = p->v_stride_l;
    a.bsz = p->bsz; a.n_q_heads = p->n_q_heads; a.q_len = p->q_len; a.window = p->window; a.start = start_budget;
    if (int rc = kvc::launch_cam_merge(a, p->dtype, p->head_dim, static_cast<hipStream_t>(hip_stream))) return fail(rc, "no CAM kernel for dtype %d", p->dtype);
    return hip_ok("cam merge launch");
}

__attribute__((visibility("default"))) int kvc_ragged_decode_step(const kvc_ragged_decode_params* p, const void* q, const void* k_new,
                                                                  const void* v_new, void* k_flat, void* v_flat, const int64_t* seg_off,
                                                                  const int32_t* seg_len, void* out, void* hip_stream) {
    if (!p) return fail(KVC_ERR_INVALID, "params is NULL");
    if (p->dtype < KVC_BF16 || p->dtype > KVC_FP32) return fail(KVC_ERR_INVALID, "unknown dtype %d", p->dtype);
    if (p->bsz < 1 || p->n_q_heads < 1 || p->n_kv_heads < 1 || p->n_q_heads % p->n_kv_heads) return fail(KVC_ERR_INVALID, "bsz / head counts invalid");
    if (p->head_dim != 64 && p->head_dim != 128) return fail(KVC_ERR_UNSUPPORTED, "decode kernels are built for head_dim 64 and 128, got %d", p->head_dim);
    if (p->appended < 0 || p->new_rows < 1) return fail(KVC_ERR_INVALID, "row counts invalid");
    if (!q || !k_new || !v_new || !k_flat || !v_flat || !seg_off || !seg_len || !out) return fail(KVC_ERR_INVALID, "a pointer is NULL");
    const int es = esize_of(p->dtype);
    {   // the kernels move 16-byte pieces, like kvc_decode_step's
        const void* ptrs[] = {q, k_new, v_new, k_flat, v_flat};
        for (const void* ptr : ptrs) if (((uintptr_t)ptr) % 16) return fail(KVC_ERR_ALIGNMENT, "a pointer is not 16-byte aligned");
        const int64_t strides[] = {p->q_stride_b, p->q_stride_h, p->q_stride_l, p->new_stride_b, p->new_stride_h, p->new_stride_l};
        for (int64_t sd : strides) if ((sd * es) % 16) return fail(KVC_ERR_ALIGNMENT, "a stride is not a multiple of 16 bytes");
        if (p->slack_rows > 0 && p->appended + p->new_rows > p->slack_rows)
            return fail(KVC_ERR_INVALID, "appended %d + new_rows %d exceed the %d spare rows behind every segment", p->appended, p->new_rows, p->slack_rows);
    }
    kvc::RaggedDecodeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.q = q; a.k_new = k_new; a.v_new = v_new; a.k_flat = k_flat; a.v_flat = v_flat; a.out = out; a.seg_off = seg_off; a.seg_len = seg_len;
    a.q_stride_b = p->q_stride_b; a.q_stride_h = p->q_stride_h; a.q_stride_l = p->q_stride_l;
    a.new_stride_b = p->new_stride_b; a.new_stride_h = p->new_stride_h; a.new_stride_l = p->new_stride_l;
    a.out_stride_b = p->out_stride_b; a.out_stride_h = p->out_stride_h; a.out_stride_l = p->out_stride_l;
    a.n_q_heads = p->n_q_heads; a.group = p->n_q_heads / p->n_kv_heads; a.appended = p->appended; a.new_rows = p->new_rows;
    a.esize = es; a.row_bytes = p->head_dim * es; a.scaling = p->scaling;
    if (int rc = kvc::launch_ragged_decode(a, p->dtype, p->head_dim, p->bsz * p->n_q_heads, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no ragged decode kernel for dtype %d head_dim %d", p->dtype, p->head_dim);
    return hip_ok("ragged decode launch");
}

__attribute__((visibility("default"))) int kvc_compress(const kvc_params* p, const void* q, const void* k, const void* v,
                                                        void* k_out, void* v_out, int64_t* idx_out, void* scores_out,
                                                        void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = validate(p, true)) return rc;
    if ((p->debug_stage_mask & 7) != 0) return fail(KVC_ERR_INVALID, "debug_stage_mask bits 0-2 are only honoured by kvc_scores / kvc_compress_batch");
    Items it;
    std::memset(&it, 0, sizeof(it));
    it.n = 1;
    it.q[0] = q; it.k[0] = k; it.v[0] = v; it.k_out[0] = k_out; it.v_out[0] = v_out;
    it.idx[0] = idx_out; it.scores[0] = scores_out; it.keep[0] = p->k; it.out_stride_h[0] = p->out_stride_h;
    if (ragged(p->method)) return fail(KVC_ERR_INVALID, "AdaKV / HeadKV produce a ragged cache: use the kvc_ragged_* entry points");
    return run_items(p, it, workspace, workspace_bytes, static_cast<hipStream_t>(hip_stream));
}

__attribute__((visibility("default"))) int kvc_compress_batch(const kvc_params* p, int n_items, const int32_t* k_per_item,
                                                              const void* const* q, const void* const* k, const void* const* v,
                                                              void* const* k_out, void* const* v_out, int64_t* const* idx_out,
                                                              void* const* scores_out, const int64_t* out_stride_h_per_item,
                                                              void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = validate(p, true)) return rc;
    if (n_items < 1 || !k_per_item || !k || !v || !k_out || !v_out) return fail(KVC_ERR_INVALID, "n_items >= 1 and the pointer arrays must be non-NULL");
    if (scoring(p->method) && !q) return fail(KVC_ERR_INVALID, "q array must be non-NULL for scoring methods");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // chunks of KVC_MAX_ITEMS items share one launch of each kernel; each chunk uses the same workspace (stream-ordered)
    for (int base = 0; base < n_items; base += kvc::KVC_MAX_ITEMS) {
        Items it;
        std::memset(&it, 0, sizeof(it));
        it.n = n_items - base < kvc::KVC_MAX_ITEMS ? n_items - base : kvc::KVC_MAX_ITEMS;
        for (int i = 0; i < it.n; ++i) {
            it.q[i] = q ? q[base + i] : nullptr; it.k[i] = k[base + i]; it.v[i] = v[base + i];
            it.k_out[i] = k_out[base + i]; it.v_out[i] = v_out[base + i];
            it.idx[i] = idx_out ? idx_out[base + i] : nullptr;
            it.scores[i] = scores_out ? scores_out[base + i] : nullptr;
            it.keep[i] = k_per_item[base + i];
            it.out_stride_h[i] = out_stride_h_per_item ? out_stride_h_per_item[base + i] : p->out_stride_h;
        }
        if (int rc = run_items(p, it, workspace, workspace_bytes, st)) return rc;
    }
    return KVC_OK;
}

}  // extern "C"

// ---- decode-stage compression (kvc_decode_compress.hip) ----------------------------------------------------------------------
namespace {

inline bool dc_scoring(int method) { return method == KVC_SNAPKV || method == KVC_PYRAMIDKV; }

int dc_strides(const char* what, int es, int64_t sb, int64_t sh, int64_t rows, int heads, int head_dim) {
    if ((sb * es) % 16 || (sh * es) % 16) return fail(KVC_ERR_ALIGNMENT, "%s strides not multiples of 16 bytes", what);
    if (sh < rows * head_dim || sb < (int64_t)heads * sh)
        return fail(KVC_ERR_INVALID, "%s strides (%lld, %lld) smaller than its [heads=%d][rows=%lld][head_dim=%d] extent", what, (long long)sb,
                    (long long)sh, heads, (long long)rows, head_dim);
    return KVC_OK;
}

// Every field of the params, before any pointer is looked at.
int dc_check(const kvc_decode_compress_params* p) {
    if (!p) return fail(KVC_ERR_INVALID, "params is NULL");
    if (p->method != KVC_SNAPKV && p->method != KVC_PYRAMIDKV && p->method != KVC_STREAMINGLLM)
        return fail(KVC_ERR_INVALID, "decode compression: method %d is not SnapKV, PyramidKV or StreamingLLM", p->method);
    if (p->dtype < KVC_BF16 || p->dtype > KVC_FP32) return fail(KVC_ERR_INVALID, "unknown dtype %d", p->dtype);
    if (p->bsz < 1 || p->n_q_heads < 1 || p->n_kv_heads < 1) return fail(KVC_ERR_INVALID, "bsz / head counts must be positive");
    if (p->n_q_heads % p->n_kv_heads) return fail(KVC_ERR_INVALID, "n_q_heads %d not a multiple of n_kv_heads %d", p->n_q_heads, p->n_kv_heads);
    if (p->head_dim != 64 && p->head_dim != 128) return fail(KVC_ERR_UNSUPPORTED, "decode compression is built for head_dim 64 and 128, got %d", p->head_dim);
    if (p->window < 1) return fail(KVC_ERR_INVALID, "window must be >= 1");
    if (p->window > 64) return fail(KVC_ERR_UNSUPPORTED, "scoring window %d > 64 not built", p->window);
    if (p->prefix_rows < 0) return fail(KVC_ERR_INVALID, "prefix_rows %d must be >= 0", p->prefix_rows);
    if (p->tail_rows < p->window) return fail(KVC_ERR_INVALID, "tail_rows %d < window %d: the window rows come from the tail", p->tail_rows, p->window);
    const int64_t L = (int64_t)p->prefix_rows + p->tail_rows;
    if (L > 0x7fffffffLL) return fail(KVC_ERR_INVALID, "prefix_rows + tail_rows overflows int32");
    if (L <= p->window) return fail(KVC_ERR_INVALID, "q_len %lld must exceed window %d", (long long)L, p->window);
    if (p->k < 0 || p->k > L - p->window)
        return fail(KVC_ERR_INVALID, "k=%d outside [0, q_len-window=%lld] (reference: topk k out of range)", p->k, (long long)(L - p->window));
    if (p->tie_mode != KVC_TIES_TORCH_CPU && p->tie_mode != KVC_TIES_CANONICAL) return fail(KVC_ERR_INVALID, "unknown tie_mode %d", p->tie_mode);
    const int es = esize_of(p->dtype), D = p->head_dim;
    if (dc_scoring(p->method)) {
        if (p->pooling != KVC_POOL_AVG && p->pooling != KVC_POOL_MAX && p->pooling != KVC_POOL_NONE)
            return fail(KVC_ERR_INVALID, "Pooling method not supported");
        if (p->pooling != KVC_POOL_NONE) {
            if (p->kernel_size < 1 || p->kernel_size > 63) return fail(KVC_ERR_UNSUPPORTED, "kernel_size %d outside [1,63]", p->kernel_size);
            if ((p->kernel_size & 1) == 0)
                return fail(KVC_ERR_UNSUPPORTED, "even kernel_size %d: the reference's pooled length becomes n+1 and its gather can index out of range", p->kernel_size);
        }
        if (p->ring_start < 0 || p->ring_start >= p->window) return fail(KVC_ERR_INVALID, "ring_start %d outside [0, window=%d)", p->ring_start, p->window);
        const int64_t n_sel = L - p->window;
        if (p->tie_mode == KVC_TIES_CANONICAL) {
            if (p->k > 16384) return fail(KVC_ERR_UNSUPPORTED, "tie_mode canonical: k=%d > 16384 (the LDS sort of the selected set) not built", p->k);
            if (n_sel > 131072) return fail(KVC_ERR_UNSUPPORTED, "tie_mode canonical: more than 131072 candidates per head not built (torch_cpu has no such limit)");
        } else if ((int64_t)p->k * 64 <= n_sel && p->k > 18000) {
            return fail(KVC_ERR_UNSUPPORTED, "tie_mode torch_cpu: a partial_sort heap of k=%d does not fit in LDS", p->k);
        }
        if (int rc = dc_strides("ring", es, p->ring_stride_b, p->ring_stride_h, p->window, p->n_q_heads, D)) return rc;
    }
    if (p->prefix_rows > 0)
        if (int rc = dc_strides("prefix", es, p->prefix_stride_b, p->prefix_stride_h, p->prefix_rows, p->n_q_heads, D)) return rc;
    if (int rc = dc_strides("tail", es, p->tail_stride_b, p->tail_stride_h, p->tail_rows, p->n_kv_heads, D)) return rc;
    if (int rc = dc_strides("out", es, p->out_stride_b, p->out_stride_h, (int64_t)p->k + p->window, p->n_q_heads, D)) return rc;
    return KVC_OK;
}

// kvc_params of the equivalent kvc_compress call, for the workspace layout and the selection.  n_kv_heads stays H_kv (the
// materialised K would have H_q): carve() reads it only to pick its tile count, the scan takes at most that many partitions,
// and the row-maxima region is sized by bsz * H_q * tile count either way.
kvc_params dc_as_compress(const kvc_decode_compress_params* p) {
    kvc_params c;
    std::memset(&c, 0, sizeof(c));
    c.method = p->method; c.dtype = p->dtype; c.bsz = p->bsz; c.n_q_heads = p->n_q_heads; c.n_kv_heads = p->n_kv_heads;
    c.q_len = p->prefix_rows + p->tail_rows; c.head_dim = p->head_dim; c.window = p->window; c.k = p->k;
    c.kernel_size = p->kernel_size; c.pooling = p->pooling; c.tie_mode = p->tie_mode; c.dot_mode = KVC_DOT_EXACT;
    return c;
}

size_t dc_workspace(const kvc_params& c) {
    if (!dc_scoring(c.method)) return 0;
    return carve(&c).total + exact_scratch_total(&c, 1, &c.k);
}

struct Span { uintptr_t lo, hi; };
Span dc_span(const void* ptr, int64_t sb, int64_t sh, int bsz, int heads, int64_t rows, int head_dim, int es) {
    const uintptr_t lo = (uintptr_t)ptr;
    return {lo, lo + (uintptr_t)(((int64_t)(bsz - 1) * sb + (int64_t)(heads - 1) * sh + rows * head_dim) * es)};
}
inline bool overlaps(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" {

__attribute__((visibility("default"))) size_t kvc_decode_compress_workspace_bytes(const kvc_decode_compress_params* p) {
    if (dc_check(p) != KVC_OK) return 0;
    g_err[0] = 0;
    const kvc_params c = dc_as_compress(p);
    return dc_workspace(c);
}

__attribute__((visibility("default"))) int kvc_decode_compress(const kvc_decode_compress_params* p, const void* q_ring, const void* k_prefix,
                                                               const void* v_prefix, const void* k_tail, const void* v_tail, void* k_out,
                                                               void* v_out, int64_t* idx_out, void* scores_out, void* workspace,
                                                               size_t workspace_bytes, void* hip_stream) {
    if (int rc = dc_check(p)) return rc;
    const bool sc = dc_scoring(p->method);
    const int es = esize_of(p->dtype), D = p->head_dim, P = p->prefix_rows, T = p->tail_rows, W = p->window;
    const int L = P + T, G = p->n_q_heads / p->n_kv_heads;
    if (!k_tail || !v_tail || !k_out || !v_out) return fail(KVC_ERR_INVALID, "k_tail, v_tail, k_out and v_out must be non-NULL");
    if (P > 0 && (!k_prefix || !v_prefix)) return fail(KVC_ERR_INVALID, "k_prefix and v_prefix must be non-NULL when prefix_rows > 0");
    if (sc && !q_ring) return fail(KVC_ERR_INVALID, "q_ring must be non-NULL for scoring methods");
    if (((uintptr_t)k_tail | (uintptr_t)v_tail | (uintptr_t)k_out | (uintptr_t)v_out) % 16 ||
        (P > 0 && ((uintptr_t)k_prefix | (uintptr_t)v_prefix) % 16) || (sc && ((uintptr_t)q_ring) % 16))
        return fail(KVC_ERR_ALIGNMENT, "q_ring / k_prefix / v_prefix / k_tail / v_tail / k_out / v_out not 16-byte aligned");
    if (!sc && idx_out && p->k > 0)
        return fail(KVC_ERR_UNSUPPORTED, "StreamingLLM: idx_out must be NULL (indices are arange(k), pyramidkv_utils.py:607)");
    if ((idx_out && ((uintptr_t)idx_out) % 16) || (sc && scores_out && ((uintptr_t)scores_out) % 16))
        return fail(KVC_ERR_ALIGNMENT, "idx_out / scores_out not 16-byte aligned");
    {   // the output never aliases the input (nor K' the V')
        const Span ko = dc_span(k_out, p->out_stride_b, p->out_stride_h, p->bsz, p->n_q_heads, p->k + W, D, es);
        const Span vo = dc_span(v_out, p->out_stride_b, p->out_stride_h, p->bsz, p->n_q_heads, p->k + W, D, es);
        const Span kt = dc_span(k_tail, p->tail_stride_b, p->tail_stride_h, p->bsz, p->n_kv_heads, T, D, es);
        const Span vt = dc_span(v_tail, p->tail_stride_b, p->tail_stride_h, p->bsz, p->n_kv_heads, T, D, es);
        bool bad = overlaps(ko, vo) || overlaps(ko, kt) || overlaps(ko, vt) || overlaps(vo, kt) || overlaps(vo, vt);
        if (P > 0) {
            const Span kp = dc_span(k_prefix, p->prefix_stride_b, p->prefix_stride_h, p->bsz, p->n_q_heads, P, D, es);
            const Span vp = dc_span(v_prefix, p->prefix_stride_b, p->prefix_stride_h, p->bsz, p->n_q_heads, P, D, es);
            bad = bad || overlaps(ko, kp) || overlaps(ko, vp) || overlaps(vo, kp) || overlaps(vo, vp);
        }
        if (bad) return fail(KVC_ERR_INVALID, "k_out / v_out overlap each other, the prefix or the tail (alternate two prefix buffers)");
    }
    const kvc_params c = dc_as_compress(p);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(workspace);
    int64_t* idx = nullptr;
    if (sc) {
        const Layout l = carve(&c);
        const size_t need = dc_workspace(c);
        if (!workspace) return fail(KVC_ERR_WORKSPACE, "workspace is NULL, need %zu bytes", need);
        if (((uintptr_t)workspace) % 256) return fail(KVC_ERR_WORKSPACE, "workspace must be 256-byte aligned");
        if (workspace_bytes < need) return fail(KVC_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, need);
        // stage 1: the two-segment window scan -> logits + partition maxima in kvc_compress's workspace layout
        const int n_parts = l.n_tiles < (L + 255) / 256 ? l.n_tiles : (L + 255) / 256;   // <= the layout's tile count, >= 1
        kvc::DcScanArgs s;
        std::memset(&s, 0, sizeof(s));
        s.ring = q_ring; s.kp = k_prefix; s.kt = k_tail;
        s.ring_sb = p->ring_stride_b; s.ring_sh = p->ring_stride_h;
        s.kp_sb = p->prefix_stride_b; s.kp_sh = p->prefix_stride_h; s.kt_sb = p->tail_stride_b; s.kt_sh = p->tail_stride_h;
        s.logits = ws + l.logits; s.pmax = reinterpret_cast<float*>(ws + l.pmax);
        s.n_q_heads = p->n_q_heads; s.group = G; s.prefix_rows = P; s.q_len = L; s.window = W; s.ring_start = p->ring_start;
        s.n_parts = n_parts; s.keys_per_part = (L + n_parts - 1) / n_parts;
        s.sqrt_d = (float)std::sqrt((double)D);                 // math.sqrt(head_dim) -> fp32 (pyramidkv_utils.py:317)
        if (int rc = kvc::launch_dc_scan(s, p->dtype, D, p->bsz, st)) return fail(rc, "no decode scan kernel for dtype %d head_dim %d", p->dtype, D);
        if (int rc = hip_ok("decode compress scan launch")) return rc;
        // stage 2: kvc_compress's softmax / window sum / pooling over those logits (stage mask 6: the K-scan is not enqueued)
        void* scores = scores_out ? scores_out : ws + l.scores;
        kvc::ScoreArgs a;
        std::memset(&a, 0, sizeof(a));
        a.scores.p[0] = scores;
        a.n_items = 1;
        a.ws = ws; a.ws_item_stride = (int64_t)l.total;
        a.off_logits = (int64_t)l.logits; a.off_pmax = (int64_t)l.pmax;
        a.off_rowmax = (int64_t)l.rowmax; a.off_rowsum = (int64_t)l.rowsum;
        a.off_part16 = l.has_part16 ? (int64_t)l.psum : -1;
        a.bsz = p->bsz; a.n_q_heads = p->n_q_heads; a.n_kv_heads = p->n_kv_heads; a.group = G;
        a.q_len = L; a.window = W; a.n_tiles = n_parts;
        a.kernel_size = p->kernel_size; a.pooling = p->pooling;
        a.stage_mask = 6;
        a.sqrt_d = s.sqrt_d;
        if (int rc = kvc::launch_scores(a, p->dtype, D, st)) return fail(rc, "no scoring kernel for dtype %d head_dim %d", p->dtype, D);
        if (int rc = hip_ok("decode compress softmax launch")) return rc;
        // stage 3: the selection (never the fused select + gather: it has one gather source)
        idx = idx_out ? idx_out : reinterpret_cast<int64_t*>(ws + l.idx);
        if (p->k > 0) {
            Items it;
            std::memset(&it, 0, sizeof(it));
            it.n = 1; it.scores[0] = scores; it.idx[0] = idx; it.keep[0] = p->k; it.k_max = p->k;
            if (int rc = enqueue_select(&c, it, false, ws + l.total, st)) return rc;
        }
    }
    // stage 4: the two-source gather (StreamingLLM: this alone, identity indices)
    kvc::DcGatherArgs g;
    std::memset(&g, 0, sizeof(g));
    g.src_p[0] = k_prefix; g.src_p[1] = v_prefix; g.src_t[0] = k_tail; g.src_t[1] = v_tail; g.out[0] = k_out; g.out[1] = v_out;
    g.idx = sc ? idx : nullptr;
    g.p_sb = p->prefix_stride_b; g.p_sh = p->prefix_stride_h; g.t_sb = p->tail_stride_b; g.t_sh = p->tail_stride_h;
    g.o_sb = p->out_stride_b; g.o_sh = p->out_stride_h;
    g.n_q_heads = p->n_q_heads; g.group = G; g.prefix_rows = P; g.q_len = L; g.window = W; g.k = p->k;
    g.esize = es; g.row_bytes = D * es;
    kvc::launch_dc_gather(g, p->bsz, st);
    return hip_ok("decode compress gather launch");
}

}  // extern "C"

// ---- heavy hitters at decode time (kvc_decode_scored.hip) ---------------------------------------------------------------------
namespace {

int score_strides(const char* what, int64_t sb, int64_t sh, int64_t rows, int heads) {
    if (sh < rows || sb < (int64_t)heads * sh)
        return fail(KVC_ERR_INVALID, "%s strides (%lld, %lld) smaller than its [heads=%d][rows=%lld] extent", what, (long long)sb, (long long)sh,
                    heads, (long long)rows);
    return KVC_OK;
}

// Every field of the params, before any pointer is looked at.
int scored_check(const kvc_decode_scored_params* sp) {
    if (!sp) return fail(KVC_ERR_INVALID, "params is NULL");
    const kvc_decode_params* p = &sp->step;
    if (int rc = decode_check(p, nullptr)) return rc;
    const int64_t rows = (int64_t)p->prefix_rows + p->tail_rows + p->new_rows;
    if (rows > 0x7fffffffLL) return fail(KVC_ERR_INVALID, "prefix_rows + tail_rows + new_rows overflows int32");
    const int es = esize_of(p->dtype);
    const int64_t strides[] = {p->q_stride_b, p->q_stride_h, p->q_stride_l, p->new_stride_b, p->new_stride_h, p->new_stride_l,
                               p->prefix_stride_b, p->prefix_stride_h, p->tail_stride_b, p->tail_stride_h};
    for (int64_t sd : strides) if ((sd * es) % 16) return fail(KVC_ERR_ALIGNMENT, "a stride is not a multiple of 16 bytes");
    if (p->prefix_rows > 0)
        if (int rc = score_strides("score_prefix", sp->score_prefix_stride_b, sp->score_prefix_stride_h, p->prefix_rows, p->n_q_heads)) return rc;
    if (int rc = score_strides("score_tail", sp->score_tail_stride_b, sp->score_tail_stride_h, (int64_t)p->tail_rows + p->new_rows, p->n_q_heads))
        return rc;
    return KVC_OK;
}

struct ScoredLayout { int splits; size_t part, logit, total; };
ScoredLayout scored_layout(const kvc_decode_params* p) {
    ScoredLayout l;
    const int rows = p->prefix_rows + p->tail_rows + p->new_rows;
    const size_t items = (size_t)p->bsz * p->n_q_heads * p->new_rows;
    l.splits = kvc::decode_splits(p->bsz, p->n_q_heads, p->new_rows, rows);                 // kvc_decode_step2's plan
    l.part = 0;
    l.logit = align_up(items * (size_t)l.splits * (p->head_dim + 2) * sizeof(float), 16);   // (M, Lsum) even with one split
    l.total = align_up(l.logit + items * (size_t)rows * sizeof(float), 16);
    return l;
}

int evict_check(const kvc_decode_evict_params* p) {
    if (!p) return fail(KVC_ERR_INVALID, "params is NULL");
    if (p->dtype < KVC_BF16 || p->dtype > KVC_FP32) return fail(KVC_ERR_INVALID, "unknown dtype %d", p->dtype);
    if (p->bsz < 1 || p->n_q_heads < 1 || p->n_kv_heads < 1) return fail(KVC_ERR_INVALID, "bsz / head counts must be positive");
    if (p->n_q_heads % p->n_kv_heads) return fail(KVC_ERR_INVALID, "n_q_heads %d not a multiple of n_kv_heads %d", p->n_q_heads, p->n_kv_heads);
    if (p->head_dim != 64 && p->head_dim != 128) return fail(KVC_ERR_UNSUPPORTED, "decode eviction is built for head_dim 64 and 128, got %d", p->head_dim);
    if (p->window < 1) return fail(KVC_ERR_INVALID, "window must be >= 1");
    if (p->prefix_rows < 0) return fail(KVC_ERR_INVALID, "prefix_rows %d must be >= 0", p->prefix_rows);
    if (p->tail_rows < p->window) return fail(KVC_ERR_INVALID, "tail_rows %d < window %d: the window rows come from the tail", p->tail_rows, p->window);
    const int64_t S = (int64_t)p->prefix_rows + p->tail_rows;
    if (S > 0x7fffffffLL) return fail(KVC_ERR_INVALID, "prefix_rows + tail_rows overflows int32");
    const int64_t n = S - p->window;
    if (p->k < 0 || p->k > n) return fail(KVC_ERR_INVALID, "k=%d outside [0, rows-window=%lld]", p->k, (long long)n);
    if (p->tie_mode != KVC_TIES_TORCH_CPU && p->tie_mode != KVC_TIES_CANONICAL) return fail(KVC_ERR_INVALID, "unknown tie_mode %d", p->tie_mode);
    if (p->tie_mode == KVC_TIES_CANONICAL) {
        if (p->k > 16384) return fail(KVC_ERR_UNSUPPORTED, "tie_mode canonical: k=%d > 16384 (the LDS sort of the selected set) not built", p->k);
        if (n > 131072) return fail(KVC_ERR_UNSUPPORTED, "tie_mode canonical: more than 131072 candidates per head not built (torch_cpu has no such limit)");
    } else if ((int64_t)p->k * 64 <= n && p->k > 18000) {
        return fail(KVC_ERR_UNSUPPORTED, "tie_mode torch_cpu: a partial_sort heap of k=%d does not fit in LDS", p->k);
    }
    const int es = esize_of(p->dtype), D = p->head_dim;
    if (p->prefix_rows > 0) {
        if (int rc = dc_strides("prefix", es, p->prefix_stride_b, p->prefix_stride_h, p->prefix_rows, p->n_q_heads, D)) return rc;
        if (int rc = score_strides("score_prefix", p->score_prefix_stride_b, p->score_prefix_stride_h, p->prefix_rows, p->n_q_heads)) return rc;
    }
    if (int rc = dc_strides("tail", es, p->tail_stride_b, p->tail_stride_h, p->tail_rows, p->n_kv_heads, D)) return rc;
    if (int rc = dc_strides("out", es, p->out_stride_b, p->out_stride_h, (int64_t)p->k + p->window, p->n_q_heads, D)) return rc;
    if (int rc = score_strides("score_tail", p->score_tail_stride_b, p->score_tail_stride_h, p->tail_rows, p->n_q_heads)) return rc;
    if (int rc = score_strides("score_out", p->score_out_stride_b, p->score_out_stride_h, (int64_t)p->k + p->window, p->n_q_heads)) return rc;
    return KVC_OK;
}

struct EvictLayout { size_t cand, idx, exact, total; };
EvictLayout evict_layout(const kvc_decode_evict_params* p) {
    EvictLayout l;
    const size_t heads = (size_t)p->bsz * p->n_q_heads, n = (size_t)p->prefix_rows + p->tail_rows - p->window;
    l.cand = 0;
    l.idx = align_up(heads * n * sizeof(float), 256);
    l.exact = align_up(l.idx + heads * (size_t)p->k * 8, 256);
    const size_t ex = (p->tie_mode == KVC_TIES_TORCH_CPU && p->k > 0) ? kvc::select_exact_scratch_bytes((int)heads, (int)n, p->k) : 0;
    l.total = l.exact + align_up(ex, 256);
    return l;
}

Span score_span(const float* ptr, int64_t sb, int64_t sh, int bsz, int heads, int64_t rows) {
    const uintptr_t lo = (uintptr_t)ptr;
    return {lo, lo + (uintptr_t)(((int64_t)(bsz - 1) * sb + (int64_t)(heads - 1) * sh + rows) * 4)};
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) size_t kvc_decode_scored_workspace_bytes(const kvc_decode_scored_params* p) {
    if (scored_check(p) != KVC_OK) return 0;
    g_err[0] = 0;
    return scored_layout(&p->step).total;
}

__attribute__((visibility("default"))) int kvc_decode_step_scored(const kvc_decode_scored_params* sp, const void* q, const void* k_new,
                                                                  const void* v_new, const void* k_prefix, const void* v_prefix, void* k_tail,
                                                                  void* v_tail, float* score_prefix, float* score_tail, void* out,
                                                                  void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = scored_check(sp)) return rc;
    const kvc_decode_params* p = &sp->step;
    if (!q || !k_new || !v_new || !k_tail || !v_tail || !out || !score_tail || (p->prefix_rows > 0 && (!k_prefix || !v_prefix || !score_prefix)))
        return fail(KVC_ERR_INVALID, "q, k_new, v_new, the tail, score_tail, out (and the prefix and score_prefix when it has rows) must be non-NULL");
    const void* ptrs[] = {q, k_new, v_new, k_tail, v_tail, p->prefix_rows > 0 ? k_prefix : nullptr, p->prefix_rows > 0 ? v_prefix : nullptr};
    for (const void* ptr : ptrs) if (((uintptr_t)ptr) % 16) return fail(KVC_ERR_ALIGNMENT, "a pointer is not 16-byte aligned");
    if (((uintptr_t)score_tail) % 4 || (p->prefix_rows > 0 && ((uintptr_t)score_prefix) % 4))
        return fail(KVC_ERR_ALIGNMENT, "score_prefix / score_tail not 4-byte aligned");
    const ScoredLayout l = scored_layout(p);
    if (!workspace) return fail(KVC_ERR_WORKSPACE, "workspace is NULL, need %zu bytes", l.total);
    if (((uintptr_t)workspace) % 16) return fail(KVC_ERR_WORKSPACE, "workspace must be 16-byte aligned");
    if (workspace_bytes < l.total) return fail(KVC_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, l.total);
    const int es = esize_of(p->dtype);
    kvc::DecodeScoredArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    kvc::DecodeArgs& a = sa.a;
    a.q = q; a.k_new = k_new; a.v_new = v_new; a.k_prefix = k_prefix; a.v_prefix = v_prefix; a.k_tail = k_tail; a.v_tail = v_tail; a.out = out;
    a.q_stride_b = p->q_stride_b; a.q_stride_h = p->q_stride_h; a.q_stride_l = p->q_stride_l;
    a.new_stride_b = p->new_stride_b; a.new_stride_h = p->new_stride_h; a.new_stride_l = p->new_stride_l;
    a.prefix_stride_b = p->prefix_stride_b; a.prefix_stride_h = p->prefix_stride_h;
    a.vprefix_stride_b = p->prefix_stride_b; a.vprefix_stride_h = p->prefix_stride_h;
    a.tail_stride_b = p->tail_stride_b; a.tail_stride_h = p->tail_stride_h;
    a.out_stride_b = p->out_stride_b; a.out_stride_h = p->out_stride_h; a.out_stride_l = p->out_stride_l;
    a.bsz = p->bsz; a.n_q_heads = p->n_q_heads; a.n_kv_heads = p->n_kv_heads; a.group = p->n_q_heads / p->n_kv_heads;
    a.prefix_rows = p->prefix_rows; a.tail_rows = p->tail_rows; a.new_rows = p->new_rows;
    a.esize = es; a.row_bytes = p->head_dim * es; a.scaling = p->scaling;
    a.splits = l.splits;
    a.part = reinterpret_cast<float*>(static_cast<char*>(workspace) + l.part);
    sa.logit = reinterpret_cast<float*>(static_cast<char*>(workspace) + l.logit);
    sa.score_prefix = score_prefix; sa.score_tail = score_tail;
    sa.sp_sb = sp->score_prefix_stride_b; sa.sp_sh = sp->score_prefix_stride_h;
    sa.st_sb = sp->score_tail_stride_b; sa.st_sh = sp->score_tail_stride_h;
    if (int rc = kvc::launch_decode_step_scored(sa, p->dtype, p->head_dim, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no scored decode kernel for dtype %d head_dim %d", p->dtype, p->head_dim);
    return hip_ok("scored decode step launch");
}

__attribute__((visibility("default"))) size_t kvc_decode_evict_workspace_bytes(const kvc_decode_evict_params* p) {
    if (evict_check(p) != KVC_OK) return 0;
    g_err[0] = 0;
    return evict_layout(p).total;
}

__attribute__((visibility("default"))) int kvc_decode_evict(const kvc_decode_evict_params* p, const void* k_prefix, const void* v_prefix,
                                                            const void* k_tail, const void* v_tail, const float* score_prefix,
                                                            const float* score_tail, void* k_out, void* v_out, float* score_out,
                                                            int64_t* idx_out, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = evict_check(p)) return rc;
    const int es = esize_of(p->dtype), D = p->head_dim, P = p->prefix_rows, T = p->tail_rows, W = p->window;
    const int n = P + T - W, G = p->n_q_heads / p->n_kv_heads;
    if (!k_tail || !v_tail || !score_tail || !k_out || !v_out || !score_out)
        return fail(KVC_ERR_INVALID, "k_tail, v_tail, score_tail, k_out, v_out and score_out must be non-NULL");
    if (P > 0 && (!k_prefix || !v_prefix || !score_prefix))
        return fail(KVC_ERR_INVALID, "k_prefix, v_prefix and score_prefix must be non-NULL when prefix_rows > 0");
    if (((uintptr_t)k_tail | (uintptr_t)v_tail | (uintptr_t)k_out | (uintptr_t)v_out) % 16 || (P > 0 && ((uintptr_t)k_prefix | (uintptr_t)v_prefix) % 16))
        return fail(KVC_ERR_ALIGNMENT, "k_prefix / v_prefix / k_tail / v_tail / k_out / v_out not 16-byte aligned");
    if (((uintptr_t)score_tail | (uintptr_t)score_out) % 4 || (P > 0 && ((uintptr_t)score_prefix) % 4))
        return fail(KVC_ERR_ALIGNMENT, "score_prefix / score_tail / score_out not 4-byte aligned");
    if (idx_out && ((uintptr_t)idx_out) % 16) return fail(KVC_ERR_ALIGNMENT, "idx_out not 16-byte aligned");
    {   // the output never aliases the input
        const Span ko = dc_span(k_out, p->out_stride_b, p->out_stride_h, p->bsz, p->n_q_heads, p->k + W, D, es);
        const Span vo = dc_span(v_out, p->out_stride_b, p->out_stride_h, p->bsz, p->n_q_heads, p->k + W, D, es);
        const Span kt = dc_span(k_tail, p->tail_stride_b, p->tail_stride_h, p->bsz, p->n_kv_heads, T, D, es);
        const Span vt = dc_span(v_tail, p->tail_stride_b, p->tail_stride_h, p->bsz, p->n_kv_heads, T, D, es);
        const Span so = score_span(score_out, p->score_out_stride_b, p->score_out_stride_h, p->bsz, p->n_q_heads, p->k + W);
        const Span stl = score_span(score_tail, p->score_tail_stride_b, p->score_tail_stride_h, p->bsz, p->n_q_heads, T);
        bool bad = overlaps(ko, vo) || overlaps(ko, kt) || overlaps(ko, vt) || overlaps(vo, kt) || overlaps(vo, vt) || overlaps(so, stl);
        if (P > 0) {
            const Span kp = dc_span(k_prefix, p->prefix_stride_b, p->prefix_stride_h, p->bsz, p->n_q_heads, P, D, es);
            const Span vp = dc_span(v_prefix, p->prefix_stride_b, p->prefix_stride_h, p->bsz, p->n_q_heads, P, D, es);
            const Span spr = score_span(score_prefix, p->score_prefix_stride_b, p->score_prefix_stride_h, p->bsz, p->n_q_heads, P);
            bad = bad || overlaps(ko, kp) || overlaps(ko, vp) || overlaps(vo, kp) || overlaps(vo, vp) || overlaps(so, spr);
        }
        if (bad) return fail(KVC_ERR_INVALID, "k_out / v_out / score_out overlap each other's inputs (alternate two prefix buffers, each with its scores)");
    }
    const EvictLayout l = evict_layout(p);
    if (!workspace) return fail(KVC_ERR_WORKSPACE, "workspace is NULL, need %zu bytes", l.total);
    if (((uintptr_t)workspace) % 256) return fail(KVC_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    if (workspace_bytes < l.total) return fail(KVC_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, l.total);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(workspace);
    kvc::EvictArgs a;
    std::memset(&a, 0, sizeof(a));
    a.score_p = score_prefix; a.score_t = score_tail; a.cand = reinterpret_cast<float*>(ws + l.cand); a.score_out = score_out;
    a.src_p[0] = k_prefix; a.src_p[1] = v_prefix; a.src_t[0] = k_tail; a.src_t[1] = v_tail; a.out[0] = k_out; a.out[1] = v_out;
    a.idx = idx_out ? idx_out : reinterpret_cast<int64_t*>(ws + l.idx);
    a.sp_sb = p->score_prefix_stride_b; a.sp_sh = p->score_prefix_stride_h; a.st_sb = p->score_tail_stride_b; a.st_sh = p->score_tail_stride_h;
    a.so_sb = p->score_out_stride_b; a.so_sh = p->score_out_stride_h;
    a.p_sb = p->prefix_stride_b; a.p_sh = p->prefix_stride_h; a.t_sb = p->tail_stride_b; a.t_sh = p->tail_stride_h;
    a.o_sb = p->out_stride_b; a.o_sh = p->out_stride_h;
    a.n_q_heads = p->n_q_heads; a.group = G; a.prefix_rows = P; a.n = n; a.window = W; a.k = p->k; a.esize = es; a.row_bytes = D * es;
    if (p->k > 0) {
        // stage 1: the candidates' scores as one fp32 row per head; stage 2: kvc_select's kernels on it
        kvc::launch_evict_scores(a, p->bsz, st);
        if (int rc = hip_ok("decode evict score layout launch")) return rc;
        kvc_params c;
        std::memset(&c, 0, sizeof(c));
        c.method = KVC_H2O; c.dtype = KVC_FP32; c.bsz = p->bsz; c.n_q_heads = p->n_q_heads; c.n_kv_heads = p->n_kv_heads;
        c.q_len = P + T; c.head_dim = D; c.window = W; c.k = p->k; c.tie_mode = p->tie_mode; c.dot_mode = KVC_DOT_EXACT;
        Items it;
        std::memset(&it, 0, sizeof(it));
        it.n = 1; it.scores[0] = a.cand; it.idx[0] = const_cast<int64_t*>(a.idx); it.keep[0] = p->k; it.k_max = p->k;
        if (int rc = enqueue_select(&c, it, false, ws + l.exact, st)) return rc;
    }
    // stage 3: K, V and the scores of the kept rows, each from the segment that holds it
    kvc::launch_evict_gather(a, p->bsz, st);
    return hip_ok("decode evict gather launch");
}

}  // extern "C"

// ---- the scored decode step with the lengths on the device (kvc_decode_dev_scored.hip) -------------------------------------------
namespace {

// Every field of the params and the capacity, before any pointer is looked at: kvc_decode_step_dev's, then the score strides.
int dev_scored_check(const kvc_decode_scored_params* sp, int32_t tail_capacity) {
    if (!sp) return fail(KVC_ERR_INVALID, "params is NULL");
    const kvc_decode_params* p = &sp->step;
    if (int rc = decode_dev_check(p, tail_capacity)) return rc;
    if (p->prefix_rows > 0)
        if (int rc = score_strides("score_prefix", sp->score_prefix_stride_b, sp->score_prefix_stride_h, p->prefix_rows, p->n_q_heads)) return rc;
    return score_strides("score_tail", sp->score_tail_stride_b, sp->score_tail_stride_h, tail_capacity, p->n_q_heads);
}

// (M, Lsum, acc[D]) of every split of the bound's plan — written with one split too — then the logits, one row of the bound's
// length per (batch row, head, token)
struct DevScoredLayout { int splits; size_t part, logit, total; };
DevScoredLayout dev_scored_layout(const kvc_decode_params* p, int32_t tail_capacity) {
    DevScoredLayout l;
    const int rows = p->prefix_rows + tail_capacity;
    const size_t items = (size_t)p->bsz * p->n_q_heads * p->new_rows;
    l.splits = kvc::decode_dev_splits(p->bsz, p->n_q_heads, p->new_rows, rows);              // kvc_decode_step_dev's plan; the launcher
    int ran = l.splits;                                                                      // rounds it to whole 64-row blocks alike
    if (ran > 1) { const int rps = ((rows + ran - 1) / ran + 63) / 64 * 64; ran = (rows + rps - 1) / rps; }
    l.part = 0;
    l.logit = align_up(items * (size_t)ran * (p->head_dim + 2) * sizeof(float), 16);
    l.total = align_up(l.logit + items * (size_t)rows * sizeof(float), 16);
    return l;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) size_t kvc_decode_dev_scored_workspace_bytes(const kvc_decode_scored_params* p, int32_t tail_capacity) {
    if (dev_scored_check(p, tail_capacity) != KVC_OK) return 0;
    g_err[0] = 0;
    return dev_scored_layout(&p->step, tail_capacity).total;
}

__attribute__((visibility("default"))) int kvc_decode_step_dev_scored(const kvc_decode_scored_params* sp, int32_t tail_capacity,
                                                                      const int32_t* tail_rows_dev, const int32_t* prefix_rows_b,
                                                                      const void* q, const void* k_new, const void* v_new,
                                                                      const void* k_prefix, const void* v_prefix, void* k_tail,
                                                                      void* v_tail, float* score_prefix, float* score_tail, void* out,
                                                                      void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = dev_scored_check(sp, tail_capacity)) return rc;
    const kvc_decode_params* p = &sp->step;
    kvc::DecodeDevScoredArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    if (int rc = decode_dev_args(p, tail_capacity, tail_rows_dev, prefix_rows_b, q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, out,
                                 nullptr, 0, sa.d)) return rc;
    if (!score_tail || (p->prefix_rows > 0 && !score_prefix))
        return fail(KVC_ERR_INVALID, "score_tail (and score_prefix when the prefix has rows) must be non-NULL");
    if (((uintptr_t)score_tail) % 4 || (p->prefix_rows > 0 && ((uintptr_t)score_prefix) % 4))
        return fail(KVC_ERR_ALIGNMENT, "score_prefix / score_tail not 4-byte aligned");
    {   // every score slot has one owner, and `out` is written while the scores are still being read
        const int es = esize_of(p->dtype);
        const uintptr_t olo = (uintptr_t)out;
        const Span so = {olo, olo + (uintptr_t)(((int64_t)(p->bsz - 1) * p->out_stride_b + (int64_t)(p->n_q_heads - 1) * p->out_stride_h +
                                                 (int64_t)(p->new_rows - 1) * p->out_stride_l + p->head_dim) * es)};
        const Span stl = score_span(score_tail, sp->score_tail_stride_b, sp->score_tail_stride_h, p->bsz, p->n_q_heads, tail_capacity);
        bool bad = overlaps(stl, so);
        if (p->prefix_rows > 0) {
            const Span spr = score_span(score_prefix, sp->score_prefix_stride_b, sp->score_prefix_stride_h, p->bsz, p->n_q_heads, p->prefix_rows);
            bad = bad || overlaps(spr, so) || overlaps(spr, stl);
        }
        if (bad) return fail(KVC_ERR_INVALID, "score_prefix / score_tail / out overlap each other");
    }
    const DevScoredLayout l = dev_scored_layout(p, tail_capacity);
    if (!workspace) return fail(KVC_ERR_WORKSPACE, "workspace is NULL, need %zu bytes", l.total);
    if (((uintptr_t)workspace) % 16) return fail(KVC_ERR_WORKSPACE, "workspace must be 16-byte aligned");
    if (workspace_bytes < l.total) return fail(KVC_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, l.total);
    sa.d.a.splits = l.splits;
    sa.d.a.part = reinterpret_cast<float*>(static_cast<char*>(workspace) + l.part);
    sa.logit = reinterpret_cast<float*>(static_cast<char*>(workspace) + l.logit);
    sa.score_prefix = score_prefix; sa.score_tail = score_tail;
    sa.sp_sb = sp->score_prefix_stride_b; sa.sp_sh = sp->score_prefix_stride_h;
    sa.st_sb = sp->score_tail_stride_b; sa.st_sh = sp->score_tail_stride_h;
    if (int rc = kvc::launch_decode_step_dev_scored(sa, p->dtype, p->head_dim, static_cast<hipStream_t>(hip_stream)))
        return fail(rc, "no device-counted scored decode kernel for dtype %d head_dim %d", p->dtype, p->head_dim);
    return hip_ok("device-counted scored decode step launch");
}

}  // extern "C"
