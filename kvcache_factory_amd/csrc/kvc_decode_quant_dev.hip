// kvc_decode_quant_dev.hip — the quantized decode step of kvc_quant.hip (KIVI form, no outliers) with BOTH GROWING LENGTHS read on
// the device, so that the step can be captured in a HIP graph and replayed while the quantized tail and the residual change.
//
// The prefix is quantized once: its rows P stay a host constant.  The quantized tail is a segment of fixed capacity and the
// residual a buffer of fixed capacity; their lengths live in two device int32 words the caller advances in stream order:
//     Tq = clamp(*qt_dev, 0, qt_capacity)                  rows of the quantized tail in use
//     Rr = clamp(*res_dev, 0, res_capacity - new_rows)     residual rows before this step
// The step's rows are appended at residual row Rr; token i sees virtual rows [0, P + Tq + Rr + i + 1) in the order prefix | quantized
// tail | residual, as decode_attention_q_kernel does.  The clamps keep every read and write inside the buffers whatever the words
// hold.  The grid is sized from the bound P + qt_capacity + res_capacity with a fixed rows_per_split (kvc_decode_dev.hip's rule): a
// workgroup whose first row lies at or behind the visible rows returns before it has loaded anything and writes NOTHING; the combine
// counts the splits that ran the same way and reads only those.  Split 0 is never empty.  The two words are read once per workgroup
// through the kernel-argument pointers (uniform addresses: scalar loads into SGPRs).  The row loop is decode_attention_q_kernel's:
// every load of an iteration issued before the first is used, x' = fmaf(code, scale, zero) in registers, the same fp32 dot, online
// softmax in the log2 domain and weighted sum; when Tq == qt_capacity and Rr + new_rows == res_capacity the plan is
// kvc_decode_step_quant's and so is every bit of `out`.
#include "kvc_common.h"
#include "kvc_launch.h"

namespace kvc {

namespace {
template <int BYTES> struct CodeWordDev;
template <> struct CodeWordDev<1> { typedef uint8_t type; };
template <> struct CodeWordDev<2> { typedef uint16_t type; };
template <> struct CodeWordDev<4> { typedef uint32_t type; };
template <> struct CodeWordDev<8> { typedef uint64_t type; };

template <int DT> __device__ __forceinline__ void widen_piece_q(const uint4& v, float* x) {
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

// rows of the quantized tail in use: the word clamped to what the segment holds
__device__ __forceinline__ int qtail_of(const DecodeQDevArgs& da) {
    const int n = *da.qt_dev;
    return n < 0 ? 0 : (n > da.qt_capacity ? da.qt_capacity : n);
}

// residual rows before this step: the word clamped so that the step's rows still fit the buffer
__device__ __forceinline__ int res_of(const DecodeQDevArgs& da) {
    const int n = *da.res_dev, hi = da.res_capacity - da.a.new_rows;
    return n < 0 ? 0 : (n > hi ? hi : n);
}
}  // namespace

// grid = (rows = new_rows, b * H_kv, 2 {K, V}), block = 64: 16-byte pieces of one row -> residual row Rr + i
__global__ __launch_bounds__(64) void decode_qdev_append_kernel(const DecodeQDevArgs da, const DecodeArgs ap) {
    const int i = blockIdx.x, bg = blockIdx.y, which = blockIdx.z;
    const int b = bg / ap.n_kv_heads, g = bg % ap.n_kv_heads;
    const int pieces = ap.row_bytes >> 4;
    const int Rr = res_of(da);
    const char* src = reinterpret_cast<const char*>(which ? ap.v_new : ap.k_new) +
        ((int64_t)b * ap.new_stride_b + (int64_t)g * ap.new_stride_h + (int64_t)i * ap.new_stride_l) * ap.esize;
    char* dst = reinterpret_cast<char*>(which ? ap.v_tail : ap.k_tail) +
        ((int64_t)b * ap.tail_stride_b + (int64_t)g * ap.tail_stride_h) * ap.esize + (int64_t)(Rr + i) * ap.row_bytes;
    for (int c = threadIdx.x; c < pieces; c += 64)
        reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(src)[c];
}

// grid = (b * H_q, new_rows, splits of the bound), block = 256 (4 waves) — decode_attention_q_kernel's mapping: LPR lanes share a
// row, lane c holds channels [c * EPL, (c + 1) * EPL) of q and acc.  Rows [0, P) are the query head's quantized prefix, [P, PQ) its
// KV head's quantized tail, [PQ, PQ + Rr + i + 1) the residual, PQ = P + Tq.
template <int DT, int D, int NB>
__global__ __launch_bounds__(256) void decode_qdev_attention_kernel(const DecodeQDevArgs da) {
    typedef typename Dt<DT>::raw raw;
    const DecodeQArgs& a = da.a;
    constexpr int ES = Dt<DT>::esize, EPL = 16 / ES, LPR = D / EPL;
    constexpr int RPW = 64 / LPR, RPI = 4 * RPW, UNR = 4;
    constexpr int CB = D * NB / 8, WB = EPL * NB / 8, F4 = EPL / 4;
    constexpr uint32_t MASK = (1u << NB) - 1u;
    typedef typename CodeWordDev<WB>::type cw_t;
    const int i = blockIdx.y;                                                // token of this step
    const int P = a.pre.rows, PQ = P + qtail_of(da), R = PQ + res_of(da) + i + 1;   // the two words: once per workgroup
    const int r_begin = blockIdx.z * a.rows_per_split;
    if (r_begin >= R) return;                                                // this split has no rows yet (whole workgroup)
    const int r_end = min(R, r_begin + a.rows_per_split);
    __shared__ float sm_m[4 * RPW], sm_l[4 * RPW];
    __shared__ float sm_acc[4 * RPW][D];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, slot = lane / LPR, c = lane % LPR;
    const int hb = blockIdx.x, b = hb / a.n_q_heads, h = hb % a.n_q_heads, g = h / a.group;
    const int G = a.gsize, vj = (c * EPL) / G, NG = D / G;
    const float scale = a.scaling * 1.44269504088896340736f;
    float qf[EPL];
    {
        const char* qrow = reinterpret_cast<const char*>(a.q) +
            ((int64_t)b * a.q_stride_b + (int64_t)h * a.q_stride_h + (int64_t)i * a.q_stride_l) * ES;
        widen_piece_q<DT>(reinterpret_cast<const uint4*>(qrow)[c], qf);
#pragma unroll
        for (int e = 0; e < EPL; ++e) qf[e] *= scale;
    }
    const uint8_t* pkc = a.pre.kc + (int64_t)b * a.pre.c_stride_b + (int64_t)h * a.pre.c_stride_h + c * WB;
    const uint8_t* pvc = a.pre.vc + (int64_t)b * a.pre.c_stride_b + (int64_t)h * a.pre.c_stride_h + c * WB;
    const float* pkm = a.pre.km + (int64_t)b * a.pre.km_stride_b + (int64_t)h * a.pre.km_stride_h + c * EPL;
    const float* pvm = a.pre.vm + (int64_t)b * a.pre.vm_stride_b + (int64_t)h * a.pre.vm_stride_h + vj * 2;
    const uint8_t* tkc = a.qt.kc + (int64_t)b * a.qt.c_stride_b + (int64_t)g * a.qt.c_stride_h + c * WB;
    const uint8_t* tvc = a.qt.vc + (int64_t)b * a.qt.c_stride_b + (int64_t)g * a.qt.c_stride_h + c * WB;
    const float* tkm = a.qt.km + (int64_t)b * a.qt.km_stride_b + (int64_t)g * a.qt.km_stride_h + c * EPL;
    const float* tvm = a.qt.vm + (int64_t)b * a.qt.vm_stride_b + (int64_t)g * a.qt.vm_stride_h + vj * 2;
    const char* kr = reinterpret_cast<const char*>(a.k_res) + ((int64_t)b * a.res_stride_b + (int64_t)g * a.res_stride_h) * ES;
    const char* vr = reinterpret_cast<const char*>(a.v_res) + ((int64_t)b * a.res_stride_b + (int64_t)g * a.res_stride_h) * ES;
    constexpr int ROWB = D * ES;
    float m = -1.0e30f, l = 0.0f, acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.0f;
    for (int r0 = r_begin; r0 < r_end; r0 += RPI * UNR) {
        cw_t kcw[UNR], vcw[UNR];
        float4 ksc[UNR][F4], kzp[UNR][F4];
        float2 vsz[UNR];
        uint4 kv[UNR], vv[UNR];
        bool valid[UNR], quant[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {                                      // every load of the iteration before the first use
            const int r = r0 + u * RPI + wave * RPW + slot;
            valid[u] = r < r_end;
            quant[u] = r < PQ;
            const bool pre = r < P;
            const int rr = pre ? r : r - P;                                  // row within its quantized segment
            const uint8_t* kcp = (pre ? pkc : tkc) + (int64_t)rr * CB;
            const uint8_t* vcp = (pre ? pvc : tvc) + (int64_t)rr * CB;
            const float* kmp = (pre ? pkm : tkm) + (int64_t)(rr / G) * 2 * D;
            const float* vmp = (pre ? pvm : tvm) + (int64_t)rr * NG * 2;
            const bool lq = valid[u] && quant[u], lf = valid[u] && !quant[u];
            kcw[u] = lq ? *reinterpret_cast<const cw_t*>(kcp) : (cw_t)0;
            vcw[u] = lq ? *reinterpret_cast<const cw_t*>(vcp) : (cw_t)0;
#pragma unroll
            for (int f = 0; f < F4; ++f) {
                ksc[u][f] = lq ? reinterpret_cast<const float4*>(kmp)[f] : make_float4(0.f, 0.f, 0.f, 0.f);
                kzp[u][f] = lq ? reinterpret_cast<const float4*>(kmp + D)[f] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            vsz[u] = lq ? *reinterpret_cast<const float2*>(vmp) : make_float2(0.f, 0.f);
            const int64_t fr = (int64_t)(r - PQ) * ROWB;
            kv[u] = lf ? reinterpret_cast<const uint4*>(kr + fr)[c] : make_uint4(0, 0, 0, 0);
            vv[u] = lf ? reinterpret_cast<const uint4*>(vr + fr)[c] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            float kf[EPL], vf[EPL];
            if (quant[u]) {
                const float* ks = reinterpret_cast<const float*>(ksc[u]);
                const float* kz = reinterpret_cast<const float*>(kzp[u]);
                const uint64_t kw = (uint64_t)kcw[u], vw = (uint64_t)vcw[u];
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    kf[e] = __builtin_fmaf((float)((uint32_t)(kw >> (e * NB)) & MASK), ks[e], kz[e]);
                    vf[e] = __builtin_fmaf((float)((uint32_t)(vw >> (e * NB)) & MASK), vsz[u].x, vsz[u].y);
                }
            } else {
                widen_piece_q<DT>(kv[u], kf);
                widen_piece_q<DT>(vv[u], vf);
            }
            float s = 0.0f;
#pragma unroll
            for (int e = 0; e < EPL; ++e) s = __builtin_fmaf(qf[e], kf[e], s);
            if constexpr (LPR > 1) s += xor_lane<1>(s);
            if constexpr (LPR > 2) s += xor_lane<2>(s);
            if constexpr (LPR > 4) s += xor_lane<4>(s);
            if constexpr (LPR > 8) s += xor_lane<8>(s);
            if constexpr (LPR > 16) s += xor_lane<16>(s);
            if (valid[u]) {
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
        if (a.splits == 1) {
            raw* out = reinterpret_cast<raw*>(a.out) + ((int64_t)b * a.out_stride_b + (int64_t)h * a.out_stride_h + (int64_t)i * a.out_stride_l);
            out[tid] = Dt<DT>::st(o / Lsum);
        } else {                                                             // (m, l, acc) of this split
            float* part = a.part + (((int64_t)hb * a.new_rows + i) * a.splits + blockIdx.z) * (D + 2);
            part[2 + tid] = o;
            if (tid == 0) { part[0] = M; part[1] = Lsum; }
        }
    }
}

// grid = (b * H_q, new_rows), block = D: the partial results of the splits that HAD rows -> out (decode_combine_kernel's sums)
template <int DT, int D>
__global__ __launch_bounds__(D) void decode_qdev_combine_kernel(const DecodeQDevArgs da) {
    typedef typename Dt<DT>::raw raw;
    const DecodeQArgs& a = da.a;
    const int hb = blockIdx.x, b = hb / a.n_q_heads, h = hb % a.n_q_heads, i = blockIdx.y, tid = threadIdx.x;
    const int R = a.pre.rows + qtail_of(da) + res_of(da) + i + 1;
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

// The split plan of the BOUND: launch_decode_step_quant's for a cache of pre.rows + qt_capacity + res_capacity rows.
// `append` carries the step's rows and the residual as decode_append_kernel's tail.
int launch_decode_step_quant_dev(DecodeQDevArgs da, int dtype, int head_dim, int nbits, const DecodeArgs& append, hipStream_t st) {
    DecodeQArgs& a = da.a;
    const int rows = a.pre.rows + da.qt_capacity + da.res_capacity;          // the bound: no step sees more
    if (a.splits < 1 || a.part == nullptr) a.splits = 1;
    a.rows_per_split = a.splits == 1 ? rows : ((rows + a.splits - 1) / a.splits + 63) / 64 * 64;
    if (a.splits > 1) a.splits = (rows + a.rows_per_split - 1) / a.rows_per_split;
    const dim3 grid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows, (unsigned)a.splits), cgrid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows);
    const dim3 agrid((unsigned)a.new_rows, (unsigned)(append.bsz * append.n_kv_heads), 2);
#define KVC_CASE(DT_, D_, NB_) if (dtype == DT_ && head_dim == D_ && nbits == NB_) { \
        hipLaunchKernelGGL(decode_qdev_append_kernel, agrid, dim3(64), 0, st, da, append); \
        hipLaunchKernelGGL((decode_qdev_attention_kernel<DT_, D_, NB_>), grid, dim3(256), 0, st, da); \
        if (a.splits > 1) hipLaunchKernelGGL((decode_qdev_combine_kernel<DT_, D_>), cgrid, dim3(D_), 0, st, da); return 0; }
    KVC_CASE(KVC_BF16, 128, 2) KVC_CASE(KVC_BF16, 128, 4) KVC_CASE(KVC_BF16, 128, 8)
    KVC_CASE(KVC_BF16, 64, 2) KVC_CASE(KVC_BF16, 64, 4) KVC_CASE(KVC_BF16, 64, 8)
    KVC_CASE(KVC_FP16, 128, 2) KVC_CASE(KVC_FP16, 128, 4) KVC_CASE(KVC_FP16, 128, 8)
    KVC_CASE(KVC_FP16, 64, 2) KVC_CASE(KVC_FP16, 64, 4) KVC_CASE(KVC_FP16, 64, 8)
    KVC_CASE(KVC_FP32, 128, 2) KVC_CASE(KVC_FP32, 128, 4) KVC_CASE(KVC_FP32, 128, 8)
    KVC_CASE(KVC_FP32, 64, 2) KVC_CASE(KVC_FP32, 64, 4) KVC_CASE(KVC_FP32, 64, 8)
#undef KVC_CASE
    return KVC_ERR_UNSUPPORTED;
}

}  // namespace kvc
