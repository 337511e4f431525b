// kvc_decode_dev_scored.hip — H2O's scored decode step (kvc_decode_scored.hip) with the LENGTHS read on the device
// (kvc_decode_dev.hip), so that a captured step keeps scoring while the cache grows: include/kvc.h, kvc_decode_step_dev_scored.
//
// Nothing the host passes depends on how many rows the cache holds.  Every kernel reads
//     T = clamp(*tail_rows_dev, 0, tail_capacity - new_rows)      and      P_b = clamp(prefix_rows_b[b], 0, prefix_rows)
// (P_b = prefix_rows when the pointer is null); token i of batch row b sees prefix rows [0, P_b) and tail rows [0, T + i + 1), and
// virtual row r is prefix row r for r < P_b, else tail row r - P_b.  The grids, rows_per_split and the row stride of the logits
// come from the BOUND prefix_rows + tail_capacity.
//
// The attention kernel is decode_dev_attention_kernel's row loop — same loads, same fmaf chain, same lane reduction, same online
// softmax and block merge, so `out` has kvc_decode_step_dev's bytes for the same plan — which also stores, as
// decode_scored_attention_kernel does, the log2-domain logit of every visible row (by lane c == 0 of the row's lane group) into
// the workspace [b * H_q][new_rows][bound] fp32, and (M, Lsum) of its split even when the plan has one split.  A workgroup whose
// first row lies at or behind the visible rows returns before it loads anything and writes NOTHING.  The scoring kernel owns one
// virtual row per thread: it counts the splits that ran as the combine does, merges their (M, Lsum) in the combine's order and adds
// exp2(s - M) / Lsum to the row's score, tokens ascending; a row the step appended starts from 0.  A thread whose row is not
// visible touches no score slot and no logit: prefix score slots [P_b, prefix_rows) and tail score slots at or past T + new_rows
// are neither read nor written.  No atomics; nothing depends on scheduling.
#include "kvc_common.h"
#include "kvc_launch.h"

namespace kvc {

namespace {
template <int DT> __device__ __forceinline__ void widen_piece_ds(const uint4& v, float* x) {
    if constexpr (DT == KVC_FP32) {
        x[0] = u2f(v.x); x[1] = u2f(v.y); x[2] = u2f(v.z); x[3] = u2f(v.w);
    } else {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = Dt<DT>::ld((uint16_t)(w[i] & 0xffffu));
            x[2 * i + 1] = Dt<DT>::ld((uint16_t)(w[i] >> 16));
        }
    }
}

// rows the tail holds before this step: the counter clamped so that the step's rows still fit the buffer
__device__ __forceinline__ int tail_of(const DecodeDevArgs& da) {
    const int n = *da.tail_dev, hi = da.tail_capacity - da.a.new_rows;
    return n < 0 ? 0 : (n > hi ? hi : n);
}

// prefix rows batch row b may see: the caller's entry clamped to what the buffers hold
__device__ __forceinline__ int prefix_of(const DecodeDevArgs& da, int b) {
    if (da.rows_b == nullptr) return da.a.prefix_rows;
    const int n = da.rows_b[b];
    return n < 0 ? 0 : (n > da.a.prefix_rows ? da.a.prefix_rows : n);
}
}  // namespace

// grid = (rows = new_rows, b * H_kv, 2 {K, V}), block = 64: 16-byte pieces of one row -> tail row T + i
__global__ __launch_bounds__(64) void decode_dev_scored_append_kernel(const DecodeDevArgs da) {
    const DecodeArgs& a = da.a;
    const int i = blockIdx.x, bg = blockIdx.y, which = blockIdx.z;
    const int b = bg / a.n_kv_heads, g = bg % a.n_kv_heads;
    const int pieces = a.row_bytes >> 4;
    const int T = tail_of(da);
    const char* src = reinterpret_cast<const char*>(which ? a.v_new : a.k_new) +
        ((int64_t)b * a.new_stride_b + (int64_t)g * a.new_stride_h + (int64_t)i * a.new_stride_l) * a.esize;
    char* dst = reinterpret_cast<char*>(which ? a.v_tail : a.k_tail) +
        ((int64_t)b * a.tail_stride_b + (int64_t)g * a.tail_stride_h) * a.esize + (int64_t)(T + i) * a.row_bytes;
    for (int c = threadIdx.x; c < pieces; c += 64)
        reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(src)[c];
}

// grid = (b * H_q, new_rows, splits of the bound), block = 256 (4 waves); LPR lanes share a row (16 bytes each)
template <int DT, int D>
__global__ __launch_bounds__(256) void decode_dev_scored_attention_kernel(const DecodeDevScoredArgs sa) {
    typedef typename Dt<DT>::raw raw;
    const DecodeDevArgs& da = sa.d;
    const DecodeArgs& a = da.a;
    constexpr int ES = Dt<DT>::esize, EPL = 16 / ES, LPR = D / EPL;
    constexpr int RPW = 64 / LPR, RPI = 4 * RPW, UNR = 4;
    constexpr int ROWB = D * ES;
    const int hb = blockIdx.x, b = hb / a.n_q_heads, h = hb % a.n_q_heads, g = h / a.group;
    const int i = blockIdx.y;                                                // token of this step
    const int P = prefix_of(da, b), R = P + tail_of(da) + i + 1;             // visible rows: prefix, then tail
    const int r_begin = blockIdx.z * a.rows_per_split;
    if (r_begin >= R) return;                                                // this split has no rows yet (whole workgroup)
    const int r_end = min(R, r_begin + a.rows_per_split);
    __shared__ float sm_m[4 * RPW], sm_l[4 * RPW];
    __shared__ float sm_acc[4 * RPW][D];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, slot = lane / LPR, c = lane % LPR;
    const float scale = a.scaling * 1.44269504088896340736f;                 // logits in the log2 domain
    float qf[EPL];
    {
        const char* qrow = reinterpret_cast<const char*>(a.q) +
            ((int64_t)b * a.q_stride_b + (int64_t)h * a.q_stride_h + (int64_t)i * a.q_stride_l) * ES;
        widen_piece_ds<DT>(reinterpret_cast<const uint4*>(qrow)[c], qf);
#pragma unroll
        for (int e = 0; e < EPL; ++e) qf[e] *= scale;
    }
    const char* kp = reinterpret_cast<const char*>(a.k_prefix) + ((int64_t)b * a.prefix_stride_b + (int64_t)h * a.prefix_stride_h) * ES;
    const char* vp = reinterpret_cast<const char*>(a.v_prefix) + ((int64_t)b * a.vprefix_stride_b + (int64_t)h * a.vprefix_stride_h) * ES;
    const char* kt = reinterpret_cast<const char*>(a.k_tail) + ((int64_t)b * a.tail_stride_b + (int64_t)g * a.tail_stride_h) * ES;
    const char* vt = reinterpret_cast<const char*>(a.v_tail) + ((int64_t)b * a.tail_stride_b + (int64_t)g * a.tail_stride_h) * ES;
    float* lg = sa.logit + ((int64_t)hb * a.new_rows + i) * sa.rows;         // this (head, token)'s logits, by virtual row
    float m = -1.0e30f, l = 0.0f, acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.0f;
    for (int r0 = r_begin; r0 < r_end; r0 += RPI * UNR) {
        uint4 kv[UNR], vv[UNR];
        bool valid[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {                                      // every load of the iteration before the first use
            const int r = r0 + u * RPI + wave * RPW + slot;
            valid[u] = r < r_end;
            const int64_t off = r < P ? (int64_t)r * ROWB : (int64_t)(r - P) * ROWB;
            const char* krow = (r < P ? kp : kt) + off;
            const char* vrow = (r < P ? vp : vt) + off;
            kv[u] = valid[u] ? reinterpret_cast<const uint4*>(krow)[c] : make_uint4(0, 0, 0, 0);
            vv[u] = valid[u] ? reinterpret_cast<const uint4*>(vrow)[c] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            float kf[EPL], vf[EPL];
            widen_piece_ds<DT>(kv[u], kf);
            widen_piece_ds<DT>(vv[u], vf);
            float s = 0.0f;
#pragma unroll
            for (int e = 0; e < EPL; ++e) s = __builtin_fmaf(qf[e], kf[e], s);
            if constexpr (LPR > 1) s += xor_lane<1>(s);
            if constexpr (LPR > 2) s += xor_lane<2>(s);
            if constexpr (LPR > 4) s += xor_lane<4>(s);
            if constexpr (LPR > 8) s += xor_lane<8>(s);
            if constexpr (LPR > 16) s += xor_lane<16>(s);
            if (valid[u]) {
                if (c == 0) lg[r0 + u * RPI + wave * RPW + slot] = s;        // the row's logit, by the one lane that owns it
                const float mn = s > m ? s : m;
                const float f = __builtin_amdgcn_exp2f(m - mn), p = __builtin_amdgcn_exp2f(s - mn);
                l = __builtin_fmaf(l, f, p);
#pragma unroll
                for (int e = 0; e < EPL; ++e) acc[e] = __builtin_fmaf(acc[e], f, p * vf[e]);
                m = mn;
            }
        }
    }
    // merge the 4 * RPW row slots of the block (a slot that saw no row holds the neutral (-1e30, 0, 0))
    const int sl = wave * RPW + slot;
    if (c == 0) { sm_m[sl] = m; sm_l[sl] = l; }
#pragma unroll
    for (int e = 0; e < EPL; ++e) sm_acc[sl][c * EPL + e] = acc[e];
    __syncthreads();
    if (tid < D) {
        float M = sm_m[0];
        for (int s_ = 1; s_ < 4 * RPW; ++s_) M = sm_m[s_] > M ? sm_m[s_] : M;
        float Lsum = 0.0f, o = 0.0f;
        for (int s_ = 0; s_ < 4 * RPW; ++s_) {
            const float f = __builtin_amdgcn_exp2f(sm_m[s_] - M);
            Lsum = __builtin_fmaf(sm_l[s_], f, Lsum);
            o = __builtin_fmaf(sm_acc[s_][tid], f, o);
        }
        float* part = a.part + (((int64_t)hb * a.new_rows + i) * a.splits + blockIdx.z) * (D + 2);
        if (tid == 0) { part[0] = M; part[1] = Lsum; }                       // the scoring stage needs them with one split too
        if (a.splits == 1) {
            raw* out = reinterpret_cast<raw*>(a.out) + ((int64_t)b * a.out_stride_b + (int64_t)h * a.out_stride_h + (int64_t)i * a.out_stride_l);
            out[tid] = Dt<DT>::st(o / Lsum);
        } else {
            part[2 + tid] = o;
        }
    }
}

// grid = (b * H_q, new_rows), block = D: the partial results of the splits that HAD rows -> out (decode_dev_combine_kernel)
template <int DT, int D>
__global__ __launch_bounds__(D) void decode_dev_scored_combine_kernel(const DecodeDevArgs da) {
    typedef typename Dt<DT>::raw raw;
    const DecodeArgs& a = da.a;
    const int hb = blockIdx.x, b = hb / a.n_q_heads, h = hb % a.n_q_heads, i = blockIdx.y, tid = threadIdx.x;
    const int R = prefix_of(da, b) + tail_of(da) + i + 1;
    int n = (R + a.rows_per_split - 1) / a.rows_per_split;                   // the attention kernel's `r_begin < R`, counted
    n = n > a.splits ? a.splits : n;
    const float* part = a.part + ((int64_t)hb * a.new_rows + i) * a.splits * (D + 2);
    float M = -1.0e30f;
    for (int s = 0; s < n; ++s) { const float ms = part[(int64_t)s * (D + 2)]; M = ms > M ? ms : M; }
    float Lsum = 0.0f, o = 0.0f;
    for (int s = 0; s < n; ++s) {
        const float* ps = part + (int64_t)s * (D + 2);
        const float f = __builtin_amdgcn_exp2f(ps[0] - M);
        Lsum = __builtin_fmaf(ps[1], f, Lsum);
        o = __builtin_fmaf(ps[2 + tid], f, o);
    }
    raw* out = reinterpret_cast<raw*>(a.out) + ((int64_t)b * a.out_stride_b + (int64_t)h * a.out_stride_h + (int64_t)i * a.out_stride_l);
    out[tid] = Dt<DT>::st(o / Lsum);
}

// grid = (ceil(bound / 256), b * H_q), block = 256: one virtual row per thread, score += softmax probability, tokens ascending.
// (M, Lsum) of a token: the splits that ran, merged in the combine's order, DS_TOK tokens at a time in LDS.  A workgroup whose
// first row is not visible to the step's last token returns whole; inside the others a thread whose row is not visible keeps the
// barriers company and touches nothing.
constexpr int DS_TOK = 64;
__global__ __launch_bounds__(256) void decode_dev_score_kernel(const DecodeDevScoredArgs sa, int part_stride) {
    const DecodeDevArgs& da = sa.d;
    const DecodeArgs& a = da.a;
    __shared__ float sm_M[DS_TOK], sm_L[DS_TOK];
    const int tid = threadIdx.x, hb = blockIdx.y, b = hb / a.n_q_heads, h = hb % a.n_q_heads;
    const int P = prefix_of(da, b), T = tail_of(da), r = blockIdx.x * 256 + tid;
    const int R = P + T + a.new_rows;                                        // rows the step's last token sees
    if ((int)(blockIdx.x * 256) >= R) return;                                // (whole workgroup)
    const bool mine = r < R;
    float* slot = nullptr;
    float score = 0.0f;
    if (mine) {
        if (r < P) slot = sa.score_prefix + (int64_t)b * sa.sp_sb + (int64_t)h * sa.sp_sh + r;
        else slot = sa.score_tail + (int64_t)b * sa.st_sb + (int64_t)h * sa.st_sh + (r - P);
        if (r < P + T) score = *slot;                                        // a row appended by this step starts from 0
    }
    for (int i0 = 0; i0 < a.new_rows; i0 += DS_TOK) {
        const int nt = min(DS_TOK, a.new_rows - i0);
        if (tid < nt) {
            const float* part = a.part + ((int64_t)hb * a.new_rows + i0 + tid) * a.splits * part_stride;
            const int vis = P + T + i0 + tid + 1;
            int n = (vis + a.rows_per_split - 1) / a.rows_per_split;         // the splits that ran for this token, as the combine counts
            n = n > a.splits ? a.splits : n;
            float M = -1.0e30f;
            for (int s = 0; s < n; ++s) { const float ms = part[(int64_t)s * part_stride]; M = ms > M ? ms : M; }
            float Lsum = 0.0f;
            for (int s = 0; s < n; ++s) {
                const float* ps = part + (int64_t)s * part_stride;
                Lsum = __builtin_fmaf(ps[1], __builtin_amdgcn_exp2f(ps[0] - M), Lsum);
            }
            sm_M[tid] = M; sm_L[tid] = Lsum;
        }
        __syncthreads();
        if (mine) {
            const float* lg = sa.logit + ((int64_t)hb * a.new_rows + i0) * sa.rows + r;
            for (int t = 0; t < nt; ++t)
                if (r < P + T + i0 + t + 1)                                  // visible to token i0 + t (its own row included)
                    score += __builtin_amdgcn_exp2f(lg[(int64_t)t * sa.rows] - sm_M[t]) / sm_L[t];
        }
        __syncthreads();
    }
    if (mine) *slot = score;
}

// The plan of the BOUND, as kvc_decode_dev.hip plans it: a.splits comes in as decode_dev_splits' answer for the bound.
int launch_decode_step_dev_scored(DecodeDevScoredArgs sa, int dtype, int head_dim, hipStream_t st) {
    DecodeDevArgs& da = sa.d;
    DecodeArgs& a = da.a;
    const int rows = a.prefix_rows + da.tail_capacity;                       // the bound: no step sees more
    if (a.splits < 1) a.splits = 1;
    a.rows_per_split = a.splits == 1 ? rows : ((rows + a.splits - 1) / a.splits + 63) / 64 * 64;
    if (a.splits > 1) a.splits = (rows + a.rows_per_split - 1) / a.rows_per_split;
    sa.rows = rows;
    const dim3 grid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows, (unsigned)a.splits), cgrid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows);
    const dim3 sgrid((unsigned)((rows + 255) / 256), (unsigned)(a.bsz * a.n_q_heads));
#define KVC_CASE(DT_, D_) if (dtype == DT_ && head_dim == D_) { \
        hipLaunchKernelGGL(decode_dev_scored_append_kernel, dim3((unsigned)a.new_rows, (unsigned)(a.bsz * a.n_kv_heads), 2), dim3(64), 0, st, da); \
        hipLaunchKernelGGL((decode_dev_scored_attention_kernel<DT_, D_>), grid, dim3(256), 0, st, sa); \
        if (a.splits > 1) hipLaunchKernelGGL((decode_dev_scored_combine_kernel<DT_, D_>), cgrid, dim3(D_), 0, st, da); \
        hipLaunchKernelGGL(decode_dev_score_kernel, sgrid, dim3(256), 0, st, sa, D_ + 2); return 0; }
    KVC_CASE(KVC_BF16, 128) KVC_CASE(KVC_BF16, 64) KVC_CASE(KVC_FP16, 128) KVC_CASE(KVC_FP16, 64)
    KVC_CASE(KVC_FP32, 128) KVC_CASE(KVC_FP32, 64)
#undef KVC_CASE
    return KVC_ERR_UNSUPPORTED;
}

}  // namespace kvc
