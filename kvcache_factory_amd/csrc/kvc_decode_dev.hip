// kvc_decode_dev.hip — the decode step of kvc_decode.hip / kvc_decode_rows.hip with the TAIL LENGTH read on the device.
//
// A decode step captured in a HIP graph replays with the kernel arguments and the grid of the step it was captured at, so
// nothing the host passes may depend on how many rows the tail holds.  Here the tail is a buffer of fixed capacity and its
// length lives in one device int32 the caller advances in stream order after the call (an in-graph add):
//     T = clamp(*tail_rows_dev, 0, tail_capacity - new_rows)
// is read by every kernel, the step's rows are appended at tail row T, and token i of batch row b sees prefix rows
// [0, P_b) and tail rows [0, T + i + 1).  The clamp keeps every read and write inside [0, tail_capacity) whatever the
// counter holds.  The grid is sized from the bound prefix_rows + tail_capacity with a fixed rows_per_split, as
// kvc_decode_rows.hip sizes it from the longest batch row: a workgroup whose first row lies at or behind the visible rows
// returns at once — before it has loaded anything — and writes NOTHING; the combine derives the number of splits that did
// run the same way and reads only those, so the workspace is never read where this step did not write it.  Split 0 is
// never empty (the step's own token is always visible).  P_b is rows_b[b] clamped to prefix_rows, or prefix_rows for every
// row when rows_b is null.  The row loop is decode_attention_kernel's: UNR * 4 * RPW rows in flight per workgroup, 16-byte
// pieces, online softmax in the log2 domain, fp32.
#include "kvc_common.h"
#include "kvc_launch.h"

namespace kvc {

namespace {
template <int DT> __device__ __forceinline__ void widen_piece(const uint4& v, float* x) {
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
__global__ __launch_bounds__(64) void decode_dev_append_kernel(const DecodeDevArgs da) {
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

// decode_dev_append_kernel plus the query ring, in the same launch.  grid = (rows = new_rows, 2 * b * H_kv + b * H_q), block = 64:
// blocks y < 2 * b * H_kv are the append's (K for the first b * H_kv, V for the rest); block y = 2 * b * H_kv + b' * H_q + h copies
// query row i of head h to ring slot (T + i) % W.  Only rows i >= new_rows - W are copied, so a slot has one writer per call.
__global__ __launch_bounds__(64) void decode_dev_append_ring_kernel(const DecodeDevRingArgs ra) {
    const DecodeDevArgs& da = ra.d;
    const DecodeArgs& a = da.a;
    const int i = blockIdx.x, y = blockIdx.y, kv_blocks = a.bsz * a.n_kv_heads;
    const int pieces = a.row_bytes >> 4;
    const int T = tail_of(da);
    const char* src;
    char* dst;
    if (y < 2 * kv_blocks) {
        const int which = y >= kv_blocks, bg = which ? y - kv_blocks : y;
        const int b = bg / a.n_kv_heads, g = bg % a.n_kv_heads;
        src = reinterpret_cast<const char*>(which ? a.v_new : a.k_new) +
            ((int64_t)b * a.new_stride_b + (int64_t)g * a.new_stride_h + (int64_t)i * a.new_stride_l) * a.esize;
        dst = reinterpret_cast<char*>(which ? a.v_tail : a.k_tail) +
            ((int64_t)b * a.tail_stride_b + (int64_t)g * a.tail_stride_h) * a.esize + (int64_t)(T + i) * a.row_bytes;
    } else {
        if (i < a.new_rows - ra.ring_rows) return;                           // an older row of this step: its slot belongs to a later one
        const int bh = y - 2 * kv_blocks, b = bh / a.n_q_heads, h = bh % a.n_q_heads;
        const int slot = (T + i) % ra.ring_rows;                             // T + i >= 0
        src = reinterpret_cast<const char*>(a.q) +
            ((int64_t)b * a.q_stride_b + (int64_t)h * a.q_stride_h + (int64_t)i * a.q_stride_l) * a.esize;
        dst = reinterpret_cast<char*>(ra.ring) +
            ((int64_t)b * ra.ring_stride_b + (int64_t)h * ra.ring_stride_h) * a.esize + (int64_t)slot * a.row_bytes;
    }
    for (int c = threadIdx.x; c < pieces; c += 64)
        reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(src)[c];
}

// grid = (b * H_q, new_rows, splits of the bound), block = 256 (4 waves); LPR lanes share a row (16 bytes each)
template <int DT, int D>
__global__ __launch_bounds__(256) void decode_dev_attention_kernel(const DecodeDevArgs da) {
    typedef typename Dt<DT>::raw raw;
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
        widen_piece<DT>(reinterpret_cast<const uint4*>(qrow)[c], qf);
#pragma unroll
        for (int e = 0; e < EPL; ++e) qf[e] *= scale;
    }
    const char* kp = reinterpret_cast<const char*>(a.k_prefix) + ((int64_t)b * a.prefix_stride_b + (int64_t)h * a.prefix_stride_h) * ES;
    const char* vp = reinterpret_cast<const char*>(a.v_prefix) + ((int64_t)b * a.vprefix_stride_b + (int64_t)h * a.vprefix_stride_h) * ES;
    const char* kt = reinterpret_cast<const char*>(a.k_tail) + ((int64_t)b * a.tail_stride_b + (int64_t)g * a.tail_stride_h) * ES;
    const char* vt = reinterpret_cast<const char*>(a.v_tail) + ((int64_t)b * a.tail_stride_b + (int64_t)g * a.tail_stride_h) * ES;
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
            widen_piece<DT>(kv[u], kf);
            widen_piece<DT>(vv[u], vf);
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

// grid = (b * H_q, new_rows), block = D: the partial results of the splits that HAD rows -> out
template <int DT, int D>
__global__ __launch_bounds__(D) void decode_dev_combine_kernel(const DecodeDevArgs da) {
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

// The split plan of the BOUND (rows = prefix_rows + tail_capacity): kvc_decode_step2's for one sequence, kvc_decode_step_rows'
// for a batch — the plans those entries would choose for a cache as long as this one can become.
int decode_dev_splits(int bsz, int n_q_heads, int new_rows, int rows) {
    return bsz > 1 ? decode_rows_splits(bsz, n_q_heads, new_rows, rows) : decode_splits(bsz, n_q_heads, new_rows, rows);
}

namespace {
// a.splits: the splits the workspace handed over can hold (1 without one); the bound fixes rows_per_split and the grid
void plan_of_bound(DecodeDevArgs& da) {
    DecodeArgs& a = da.a;
    const int rows = a.prefix_rows + da.tail_capacity;                       // the bound: no step sees more
    if (a.splits < 1 || a.part == nullptr) a.splits = 1;
    a.rows_per_split = a.splits == 1 ? rows : ((rows + a.splits - 1) / a.splits + 63) / 64 * 64;
    if (a.splits > 1) a.splits = (rows + a.rows_per_split - 1) / a.rows_per_split;
}
}  // namespace

// launch_decode_step_dev with the ring rows written by the append launch: the same number of launches, the same attention and
// combine kernels with the same arguments
int launch_decode_step_dev_ring(DecodeDevRingArgs ra, int dtype, int head_dim, hipStream_t st) {
    plan_of_bound(ra.d);
    const DecodeDevArgs& da = ra.d;
    const DecodeArgs& a = da.a;
    const dim3 grid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows, (unsigned)a.splits), cgrid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows);
    const dim3 agrid((unsigned)a.new_rows, (unsigned)(a.bsz * (2 * a.n_kv_heads + a.n_q_heads)));
#define KVC_CASE(DT_, D_) if (dtype == DT_ && head_dim == D_) { \
        hipLaunchKernelGGL(decode_dev_append_ring_kernel, agrid, dim3(64), 0, st, ra); \
        hipLaunchKernelGGL((decode_dev_attention_kernel<DT_, D_>), grid, dim3(256), 0, st, da); \
        if (a.splits > 1) hipLaunchKernelGGL((decode_dev_combine_kernel<DT_, D_>), cgrid, dim3(D_), 0, st, da); return 0; }
    KVC_CASE(KVC_BF16, 128) KVC_CASE(KVC_BF16, 64) KVC_CASE(KVC_FP16, 128) KVC_CASE(KVC_FP16, 64)
    KVC_CASE(KVC_FP32, 128) KVC_CASE(KVC_FP32, 64)
#undef KVC_CASE
    return KVC_ERR_UNSUPPORTED;
}

int launch_decode_step_dev(DecodeDevArgs da, int dtype, int head_dim, hipStream_t st) {
    plan_of_bound(da);
    const DecodeArgs& a = da.a;
    const dim3 grid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows, (unsigned)a.splits), cgrid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows);
#define KVC_CASE(DT_, D_) if (dtype == DT_ && head_dim == D_) { \
        hipLaunchKernelGGL(decode_dev_append_kernel, dim3((unsigned)a.new_rows, (unsigned)(a.bsz * a.n_kv_heads), 2), dim3(64), 0, st, da); \
        hipLaunchKernelGGL((decode_dev_attention_kernel<DT_, D_>), grid, dim3(256), 0, st, da); \
        if (a.splits > 1) hipLaunchKernelGGL((decode_dev_combine_kernel<DT_, D_>), cgrid, dim3(D_), 0, st, da); return 0; }
    KVC_CASE(KVC_BF16, 128) KVC_CASE(KVC_BF16, 64) KVC_CASE(KVC_FP16, 128) KVC_CASE(KVC_FP16, 64)
    KVC_CASE(KVC_FP32, 128) KVC_CASE(KVC_FP32, 64)
#undef KVC_CASE
    return KVC_ERR_UNSUPPORTED;
}

}  // namespace kvc
