// kvc_decode_scored.hip — H2O at decode time (include/kvc.h: kvc_decode_step_scored, kvc_decode_evict).
//
// H2O keeps, per query head, a running sum of the attention every later query paid to each cached row and evicts the rows
// with the smallest sums.  The sum's increment is a by-product of the decode step: the attention workgroups already hold every
// row's logit.  Here they also store it — the log2-domain logit s of row r, by lane c == 0 of the row's lane group; consecutive
// row slots hold consecutive rows, so a wave's stores coalesce — into a workspace [b * H_q][new_rows][rows] fp32, and leave
// (M, Lsum) of every split in the workspace even when there is one split only.  decode_score_kernel then owns one row per
// thread: it merges the splits' (M, Lsum) of each token exactly as decode_combine_kernel does and adds exp2(s - M) / Lsum to the
// row's score, tokens in ascending order.  No atomics, nothing depends on scheduling; rows at or behind the visible ones are
// neither read nor written, and a row appended by this step starts from 0 whatever its score slot held.
//
// The row loop is decode_attention_kernel's (kvc_decode.hip) without ThinK's pruned rows: same loads, same fmaf chain, same
// lane reduction, same online softmax and block merge, so `out` has kvc_decode_step2's bytes for the same split plan.  The
// append and the merge of the splits are that file's kernels.
//
// Eviction (kvc_decode_evict): the two score segments are laid out as one fp32 row per head, the existing selection runs on
// it (KVC_FP32 scores, either tie mode), and one gather launch copies the kept K rows, V rows and scores from the segment
// that holds each (virtual row r < P: prefix row r of the query head; else tail row r - P of its KV head — the score of a tail
// row is per QUERY head).
#include "kvc_common.h"
#include "kvc_launch.h"

namespace kvc {

namespace {
template <int DT> __device__ __forceinline__ void widen16s(const uint4& v, float* x) {
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
}  // namespace

// grid = (b * H_q, new_rows, splits), block = 256 (4 waves); LPR lanes share a row (16 bytes each)
template <int DT, int D>
__global__ __launch_bounds__(256) void decode_scored_attention_kernel(const DecodeScoredArgs sa) {
    typedef typename Dt<DT>::raw raw;
    const DecodeArgs& a = sa.a;
    constexpr int ES = Dt<DT>::esize, EPL = 16 / ES, LPR = D / EPL;
    constexpr int RPW = 64 / LPR, RPI = 4 * RPW, UNR = 4;
    constexpr int ROWB = D * ES;
    __shared__ float sm_m[4 * RPW], sm_l[4 * RPW];
    __shared__ float sm_acc[4 * RPW][D];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, slot = lane / LPR, c = lane % LPR;
    const int hb = blockIdx.x, b = hb / a.n_q_heads, h = hb % a.n_q_heads, g = h / a.group;
    const int i = blockIdx.y;                                                // token of this step
    const int P = a.prefix_rows, R = P + a.tail_rows + i + 1;                // visible rows: prefix, then tail
    const int r_begin = blockIdx.z * a.rows_per_split, r_end = min(R, r_begin + a.rows_per_split);
    const float scale = a.scaling * 1.44269504088896340736f;                 // logits in the log2 domain
    float qf[EPL];
    {
        const char* qrow = reinterpret_cast<const char*>(a.q) +
            ((int64_t)b * a.q_stride_b + (int64_t)h * a.q_stride_h + (int64_t)i * a.q_stride_l) * ES;
        widen16s<DT>(reinterpret_cast<const uint4*>(qrow)[c], qf);
#pragma unroll
        for (int e = 0; e < EPL; ++e) qf[e] *= scale;
    }
    const char* kp = reinterpret_cast<const char*>(a.k_prefix) + ((int64_t)b * a.prefix_stride_b + (int64_t)h * a.prefix_stride_h) * ES;
    const char* vp = reinterpret_cast<const char*>(a.v_prefix) + ((int64_t)b * a.vprefix_stride_b + (int64_t)h * a.vprefix_stride_h) * ES;
    const char* kt = reinterpret_cast<const char*>(a.k_tail) + ((int64_t)b * a.tail_stride_b + (int64_t)g * a.tail_stride_h) * ES;
    const char* vt = reinterpret_cast<const char*>(a.v_tail) + ((int64_t)b * a.tail_stride_b + (int64_t)g * a.tail_stride_h) * ES;
    float* lg = sa.logit + ((int64_t)hb * a.new_rows + i) * sa.rows;         // this (head, token)'s logits, one per visible row
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
            const char* krow = r < P ? kp + (int64_t)r * ROWB : kt + (int64_t)(r - P) * ROWB;
            const char* vrow = r < P ? vp + (int64_t)r * ROWB : vt + (int64_t)(r - P) * ROWB;
            kv[u] = valid[u] ? reinterpret_cast<const uint4*>(krow)[c] : make_uint4(0, 0, 0, 0);
            vv[u] = valid[u] ? reinterpret_cast<const uint4*>(vrow)[c] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            float kf[EPL], vf[EPL];
            widen16s<DT>(kv[u], kf);
            widen16s<DT>(vv[u], vf);
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

// grid = (ceil(rows / 256), b * H_q), block = 256: one row per thread, score += softmax probability, tokens ascending.
// (M, Lsum) of a token: the splits merged in decode_combine_kernel's order, SC_TOK tokens at a time in LDS.
constexpr int SC_TOK = 64;
__global__ __launch_bounds__(256) void decode_score_kernel(const DecodeScoredArgs sa, int part_stride) {
    const DecodeArgs& a = sa.a;
    __shared__ float sm_M[SC_TOK], sm_L[SC_TOK];
    const int tid = threadIdx.x, hb = blockIdx.y, b = hb / a.n_q_heads, h = hb % a.n_q_heads;
    const int P = a.prefix_rows, r = blockIdx.x * 256 + tid;
    const bool mine = r < sa.rows;
    float* slot = nullptr;
    float score = 0.0f;
    if (mine) {
        if (r < P) slot = sa.score_prefix + (int64_t)b * sa.sp_sb + (int64_t)h * sa.sp_sh + r;
        else slot = sa.score_tail + (int64_t)b * sa.st_sb + (int64_t)h * sa.st_sh + (r - P);
        if (r < P + a.tail_rows) score = *slot;                              // a row appended by this step starts from 0
    }
    for (int i0 = 0; i0 < a.new_rows; i0 += SC_TOK) {
        const int nt = min(SC_TOK, a.new_rows - i0);
        if (tid < nt) {
            const float* part = a.part + ((int64_t)hb * a.new_rows + i0 + tid) * a.splits * part_stride;
            float M = -1.0e30f;
            for (int s = 0; s < a.splits; ++s) { const float ms = part[(int64_t)s * part_stride]; M = ms > M ? ms : M; }
            float Lsum = 0.0f;
            for (int s = 0; s < a.splits; ++s) {
                const float* ps = part + (int64_t)s * part_stride;
                Lsum = __builtin_fmaf(ps[1], __builtin_amdgcn_exp2f(ps[0] - M), Lsum);
            }
            sm_M[tid] = M; sm_L[tid] = Lsum;
        }
        __syncthreads();
        if (mine) {
            const float* lg = sa.logit + ((int64_t)hb * a.new_rows + i0) * sa.rows + r;
            for (int t = 0; t < nt; ++t)
                if (r < P + a.tail_rows + i0 + t + 1)                        // visible to token i0 + t (its own row included)
                    score += __builtin_amdgcn_exp2f(lg[(int64_t)t * sa.rows] - sm_M[t]) / sm_L[t];
        }
        __syncthreads();
    }
    if (mine) *slot = score;
}

int launch_decode_step_scored(DecodeScoredArgs sa, int dtype, int head_dim, hipStream_t st) {
    DecodeArgs& a = sa.a;
    launch_decode_append(a, st);
    const int rows = a.prefix_rows + a.tail_rows + a.new_rows;
    if (a.splits < 1) a.splits = 1;                                          // kvc_decode_step2's split plan
    a.rows_per_split = a.splits == 1 ? rows : ((rows + a.splits - 1) / a.splits + 63) / 64 * 64;
    if (a.splits > 1) a.splits = (rows + a.rows_per_split - 1) / a.rows_per_split;
    sa.rows = rows;
    const dim3 grid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows, (unsigned)a.splits);
    const dim3 sgrid((unsigned)((rows + 255) / 256), (unsigned)(a.bsz * a.n_q_heads));
#define KVC_CASE(DT_, D_) if (dtype == DT_ && head_dim == D_) { hipLaunchKernelGGL((decode_scored_attention_kernel<DT_, D_>), grid, dim3(256), 0, st, sa); \
        if (a.splits > 1) launch_decode_combine(a, dtype, head_dim, st); \
        hipLaunchKernelGGL(decode_score_kernel, sgrid, dim3(256), 0, st, sa, D_ + 2); return 0; }
    KVC_CASE(KVC_BF16, 128) KVC_CASE(KVC_BF16, 64) KVC_CASE(KVC_FP16, 128) KVC_CASE(KVC_FP16, 64)
    KVC_CASE(KVC_FP32, 128) KVC_CASE(KVC_FP32, 64)
#undef KVC_CASE
    return KVC_ERR_UNSUPPORTED;
}

// ---- eviction ---------------------------------------------------------------------------------------------------------------
// grid = (ceil(n / 256), b * H_q): the candidates' scores (virtual rows [0, n), n = P + T - W) as one dense fp32 row per head
__global__ __launch_bounds__(256) void evict_scores_kernel(const EvictArgs a) {
    const int r = blockIdx.x * 256 + threadIdx.x, hb = blockIdx.y, b = hb / a.n_q_heads, h = hb % a.n_q_heads;
    if (r >= a.n) return;
    const float* src = r < a.prefix_rows ? a.score_p + (int64_t)b * a.sp_sb + (int64_t)h * a.sp_sh + r
                                         : a.score_t + (int64_t)b * a.st_sb + (int64_t)h * a.st_sh + (r - a.prefix_rows);
    a.cand[(int64_t)hb * a.n + r] = *src;
}

// dc_gather_kernel (kvc_decode_compress.hip) with the scores riding along: blockIdx.z = 0 keys, 1 values (16 bytes a lane),
// 2 the fp32 score of every output row (the first lane of the row's lane group).
__global__ __launch_bounds__(256) void evict_gather_kernel(const EvictArgs a) {
    const int which = blockIdx.z;
    const int lanes_per_row = a.row_bytes >> 4;
    const int rows_per_block = 256 / lanes_per_row;
    const int r = threadIdx.x / lanes_per_row, c = threadIdx.x % lanes_per_row;
    const int cap = a.k + a.window;
    const int t = blockIdx.x * rows_per_block + r;
    if (r >= rows_per_block || t >= cap) return;
    const int hb = blockIdx.y, b = hb / a.n_q_heads, h = hb % a.n_q_heads;
    const int D = a.row_bytes / a.esize;
    const int64_t srow = t < a.k ? a.idx[(int64_t)hb * a.k + t] : (int64_t)a.n + (t - a.k);
    const bool pre = srow < a.prefix_rows;
    if (which == 2) {
        if (c == 0) {
            const float* src = pre ? a.score_p + (int64_t)b * a.sp_sb + (int64_t)h * a.sp_sh + srow
                                   : a.score_t + (int64_t)b * a.st_sb + (int64_t)h * a.st_sh + (srow - a.prefix_rows);
            a.score_out[(int64_t)b * a.so_sb + (int64_t)h * a.so_sh + t] = *src;
        }
        return;
    }
    const char* src;
    if (pre)
        src = reinterpret_cast<const char*>(a.src_p[which]) + ((int64_t)b * a.p_sb + (int64_t)h * a.p_sh + srow * D) * a.esize;
    else
        src = reinterpret_cast<const char*>(a.src_t[which]) +
              ((int64_t)b * a.t_sb + (int64_t)(h / a.group) * a.t_sh + (srow - a.prefix_rows) * D) * a.esize;
    char* dst = reinterpret_cast<char*>(a.out[which]) + ((int64_t)b * a.o_sb + (int64_t)h * a.o_sh + (int64_t)t * D) * a.esize;
    *reinterpret_cast<uint4*>(dst + c * 16) = *reinterpret_cast<const uint4*>(src + c * 16);
}

int launch_evict_scores(const EvictArgs& a, int bsz, hipStream_t st) {
    if (a.n < 1) return 0;
    hipLaunchKernelGGL(evict_scores_kernel, dim3((unsigned)((a.n + 255) / 256), (unsigned)(bsz * a.n_q_heads)), dim3(256), 0, st, a);
    return 0;
}

int launch_evict_gather(const EvictArgs& a, int bsz, hipStream_t st) {
    const int rows_per_block = 256 / (a.row_bytes / 16);
    const int cap = a.k + a.window;
    dim3 grid((unsigned)((cap + rows_per_block - 1) / rows_per_block), (unsigned)(bsz * a.n_q_heads), 3u);
    hipLaunchKernelGGL(evict_gather_kernel, grid, dim3(256), 0, st, a);
    return 0;
}

}  // namespace kvc
