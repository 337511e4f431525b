// kvc_quant.hip — the quantized decode cache (KIVI-style; the reference's `--quant_method kivi --nbits N`).
//
// The rule, the storage layout and the entry points are described in include/kvc.h.  Three kinds of kernel:
//   quant_keys_kernel / quant_values_kernel  rows of a [b][h][row][D] source -> codes + (scale, zero); once per prompt and
//                                            once every residual_length decoded tokens (not the hot path);
//   dequant_kernel                           a segment back to [b][h][row][D] in the cache dtype (the `keys` / `values`
//                                            views and the reference-shaped decode path);
//   decode_attention_q_kernel                the hot path: decode_attention_kernel (kvc_decode.hip) over the quantized prefix,
//                                            the quantized tail and the full-precision residual; the step's rows are
//                                            appended by decode_append_kernel and the splits merged by decode_combine_kernel.
// With exact outliers (KVQuant-style, `--quant_method kvquant`): the same quantize kernels with OUTL = true zero the outliers
// before min / max and coding; outl_count_kernel / outl_scan_kernel / outl_write_kernel lay the outliers out in their pool;
// outl_patch_kernel writes them back after dequant_kernel; decode_attention_q_kernel with OUTL = true patches them in registers.
// The attention de-quantizes in registers, x' = fmaf(code, scale, zero), and then runs the same fp32 dot product / online
// softmax / weighted sum as the unquantized step: its output is attention over the de-quantized cache up to the order of
// the fp32 sums.
#include "kvc_common.h"
#include "kvc_launch.h"

namespace kvc {

template <int BYTES> struct CodeWord;
template <> struct CodeWord<1> { typedef uint8_t type; };
template <> struct CodeWord<2> { typedef uint16_t type; };
template <> struct CodeWord<4> { typedef uint32_t type; };
template <> struct CodeWord<8> { typedef uint64_t type; };

template <int NB> __device__ __forceinline__ uint32_t quant_code(float x, float mn, float sc) {
    constexpr float QMAX = (float)((1 << NB) - 1);
    if (!(sc > 0.0f)) return 0u;
    float c = __builtin_rintf((x - mn) / sc);                 // correctly rounded divide (build flags), round half to even
    c = c < 0.0f ? 0.0f : (c > QMAX ? QMAX : c);
    return (uint32_t)c;
}

// The split of include/kvc.h: thr is T' (already rounded to dtype); an outlier reads as +0 in the dense part.
__device__ __forceinline__ bool is_outlier(float x, float thr) { return x < -thr || x > thr; }
template <bool OUTL> __device__ __forceinline__ float dense(float x, float thr) {
    if constexpr (OUTL) return is_outlier(x, thr) ? 0.0f : x;
    return x;
}

// Keys: one wave per (b, h, group, 64 channels): lane = channel, min / max down its column over the group's rows (each row a
// coalesced 64-element load), then per row the lane's code, OR-ed over the CPW = 32 / NB lanes of one 32-bit word by xor
// shuffles; the word's first lane stores it.  Grid: enough 256-thread blocks for every wave item.
template <int DT, int NB, bool OUTL>
__global__ __launch_bounds__(256) void quant_keys_kernel(const QuantArgs a, const float thr) {
    typedef typename Dt<DT>::raw raw;
    constexpr int CPW = 32 / NB;
    constexpr float QMAX = (float)((1 << NB) - 1);
    const int lane = threadIdx.x & 63, CB = a.head_dim * NB / 8, WPG = a.head_dim / 64;
    const int ngroups = (a.rows + a.group - 1) / a.group;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (int64_t)a.bsz * a.n_heads * ngroups * WPG) return;         // whole waves leave together
    const int ch = (int)(item % WPG) * 64 + lane;
    int64_t t = item / WPG;
    const int grp = (int)(t % ngroups);
    t /= ngroups;
    const int h = (int)(t % a.n_heads), b = (int)(t / a.n_heads);
    const int r_lo = grp * a.group, r_hi = min(a.rows, r_lo + a.group);
    const raw* src = reinterpret_cast<const raw*>(a.src) + (int64_t)b * a.s_stride_b + (int64_t)h * a.s_stride_h + ch;
    float mn = dense<OUTL>(Dt<DT>::ld(src[(int64_t)r_lo * a.s_stride_l]), thr), mx = mn;
#pragma unroll 8
    for (int r = r_lo + 1; r < r_hi; ++r) {
        const float x = dense<OUTL>(Dt<DT>::ld(src[(int64_t)r * a.s_stride_l]), thr);
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
    }
    const float sc = (mx - mn) / QMAX;
    float* meta = a.meta + (int64_t)b * a.m_stride_b + (int64_t)h * a.m_stride_h + (int64_t)(a.row0 / a.group + grp) * 2 * a.head_dim + ch;
    meta[0] = sc;
    meta[a.head_dim] = mn;
    uint8_t* codes = a.codes + (int64_t)b * a.c_stride_b + (int64_t)h * a.c_stride_h + (int64_t)a.row0 * CB + (ch / CPW) * 4;
#pragma unroll 4
    for (int r = r_lo; r < r_hi; ++r) {
        int word = (int)(quant_code<NB>(dense<OUTL>(Dt<DT>::ld(src[(int64_t)r * a.s_stride_l]), thr), mn, sc) << ((lane % CPW) * NB));
#pragma unroll
        for (int o = 1; o < CPW; o <<= 1) word |= __shfl_xor(word, o);
        if (lane % CPW == 0) *reinterpret_cast<uint32_t*>(codes + (int64_t)r * CB) = (uint32_t)word;
    }
}

// Values: one thread per (b, h, row, channel group): min / max along the group's G channels, then its G * NB / 32 words.
template <int DT, int NB, bool OUTL>
__global__ __launch_bounds__(256) void quant_values_kernel(const QuantArgs a, const float thr) {
    typedef typename Dt<DT>::raw raw;
    constexpr int CPW = 32 / NB;
    constexpr float QMAX = (float)((1 << NB) - 1);
    const int G = a.group, NG = a.head_dim / G, CB = a.head_dim * NB / 8;
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= (int64_t)a.bsz * a.n_heads * a.rows * NG) return;
    const int j = (int)(item % NG);
    int64_t t = item / NG;
    const int r = (int)(t % a.rows);
    t /= a.rows;
    const int h = (int)(t % a.n_heads), b = (int)(t / a.n_heads);
    const raw* src = reinterpret_cast<const raw*>(a.src) + (int64_t)b * a.s_stride_b + (int64_t)h * a.s_stride_h + (int64_t)r * a.s_stride_l + j * G;
    float mn = dense<OUTL>(Dt<DT>::ld(src[0]), thr), mx = mn;
    for (int e = 1; e < G; ++e) {
        const float x = dense<OUTL>(Dt<DT>::ld(src[e]), thr);
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
    }
    const float sc = (mx - mn) / QMAX;
    const int64_t row = (int64_t)a.row0 + r;
    float* meta = a.meta + (int64_t)b * a.m_stride_b + (int64_t)h * a.m_stride_h + (row * NG + j) * 2;
    meta[0] = sc;
    meta[1] = mn;
    uint32_t* codes = reinterpret_cast<uint32_t*>(a.codes + (int64_t)b * a.c_stride_b + (int64_t)h * a.c_stride_h + row * CB + j * G * NB / 8);
    for (int wi = 0; wi < G / CPW; ++wi) {
        uint32_t word = 0;
#pragma unroll
        for (int e = 0; e < CPW; ++e) word |= quant_code<NB>(dense<OUTL>(Dt<DT>::ld(src[wi * CPW + e]), thr), mn, sc) << (e * NB);
        codes[wi] = word;
    }
}

// One thread per (b, h, row, 32-bit code word): CPW de-quantized elements of the row.
template <int DT, int NB, int MODE>
__global__ __launch_bounds__(256) void dequant_kernel(const QuantArgs a) {
    typedef typename Dt<DT>::raw raw;
    constexpr int CPW = 32 / NB;
    constexpr uint32_t MASK = (1u << NB) - 1u;
    const int NW = a.head_dim / CPW, CB = a.head_dim * NB / 8, NG = a.head_dim / a.group;
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= (int64_t)a.bsz * a.n_heads * a.rows * NW) return;
    const int w = (int)(item % NW);
    int64_t t = item / NW;
    const int r = (int)(t % a.rows);
    t /= a.rows;
    const int h = (int)(t % a.n_heads), b = (int)(t / a.n_heads);
    const int64_t row = (int64_t)a.row0 + r;
    const uint32_t word = *reinterpret_cast<const uint32_t*>(a.codes_in + (int64_t)b * a.c_stride_b + (int64_t)h * a.c_stride_h + row * CB + w * 4);
    const float* meta = a.meta_in + (int64_t)b * a.m_stride_b + (int64_t)h * a.m_stride_h;
    raw* dst = reinterpret_cast<raw*>(a.dst) + (int64_t)b * a.s_stride_b + (int64_t)h * a.s_stride_h + (int64_t)r * a.s_stride_l + w * CPW;
#pragma unroll
    for (int e = 0; e < CPW; ++e) {
        const int d = w * CPW + e;
        float sc, zp;
        if constexpr (MODE == KVC_QUANT_KEYS) {
            const float* m = meta + (row / a.group) * 2 * a.head_dim;
            sc = m[d]; zp = m[a.head_dim + d];
        } else {
            const float* m = meta + (row * NG + d / a.group) * 2;
            sc = m[0]; zp = m[1];
        }
        dst[e] = Dt<DT>::st(__builtin_fmaf((float)((word >> (e * NB)) & MASK), sc, zp));
    }
}

// ---- the sparse half: one wave per (b, h, row) of the call; lane = channel within each 64-channel chunk ----------------------
__device__ __forceinline__ int wave_item_rows(const QuantArgs& a, int& b, int& h, int& r) {
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (int64_t)a.bsz * a.n_heads * a.rows) return 0;
    r = (int)(item % a.rows);
    const int64_t t = item / a.rows;
    h = (int)(t % a.n_heads); b = (int)(t / a.n_heads);
    return 1;
}

// The row's outlier count (ballot + popcount per chunk) into its rowinfo word, for outl_scan_kernel.
template <int DT>
__global__ __launch_bounds__(256) void outl_count_kernel(const QuantArgs a, const OutlArgs o) {
    typedef typename Dt<DT>::raw raw;
    int b, h, r;
    if (!wave_item_rows(a, b, h, r)) return;
    const int lane = threadIdx.x & 63;
    const raw* src = reinterpret_cast<const raw*>(a.src) + (int64_t)b * a.s_stride_b + (int64_t)h * a.s_stride_h + (int64_t)r * a.s_stride_l;
    uint32_t cnt = 0;
    for (int c0 = 0; c0 < a.head_dim; c0 += 64)
        cnt += (uint32_t)__popcll(__ballot(is_outlier(Dt<DT>::ld(src[c0 + lane]), o.thr)));
    if (lane == 0) o.rowinfo[(int64_t)b * o.ri_stride_b + (int64_t)h * o.ri_stride_h + a.row0 + r] = cnt;
}

// One block per batch row: exclusive scan of the counts in (h, row) order from used[b]; rowinfo = (start << 8) | count for rows that
// fit below pool_capacity, 0 otherwise; used[b] += total (saturating at INT32_MAX).
__global__ __launch_bounds__(1024) void outl_scan_kernel(const QuantArgs a, const OutlArgs o) {
    __shared__ int64_t sm_wave[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = (int64_t)a.n_heads * a.rows;
    const int64_t used0 = o.used[b];
    uint32_t* ri = o.rowinfo + (int64_t)b * o.ri_stride_b + a.row0;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t idx = base + tid;
        const int h = (int)(idx / a.rows), r = (int)(idx % a.rows);
        const uint32_t cnt = idx < n ? (ri[(int64_t)h * o.ri_stride_h + r] & 0xffu) : 0u;
        int64_t x = cnt;                                               // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) sm_wave[wave] = x;
        __syncthreads();
        int64_t before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? sm_wave[w] : 0;
            total += sm_wave[w];
        }
        const int64_t start = used0 + carry + before + x - cnt;
        if (idx < n)
            ri[(int64_t)h * o.ri_stride_h + r] = (cnt > 0 && start + cnt <= o.pool_capacity) ? (uint32_t)(start << 8) | cnt : 0u;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t u = used0 + carry;
        o.used[b] = u > 0x7fffffff ? 0x7fffffff : (int32_t)u;
    }
}

// The row's entries in channel order at its start: rank = mbcnt of the chunk's ballot + the earlier chunks' popcounts.
template <int DT>
__global__ __launch_bounds__(256) void outl_write_kernel(const QuantArgs a, const OutlArgs o) {
    typedef typename Dt<DT>::raw raw;
    int b, h, r;
    if (!wave_item_rows(a, b, h, r)) return;
    const int lane = threadIdx.x & 63;
    const uint32_t word = o.rowinfo[(int64_t)b * o.ri_stride_b + (int64_t)h * o.ri_stride_h + a.row0 + r];
    const uint32_t cnt = word & 0xffu;
    if (cnt == 0) return;
    const int64_t e0 = (int64_t)b * o.pool_stride_b + (word >> 8);
    const raw* src = reinterpret_cast<const raw*>(a.src) + (int64_t)b * a.s_stride_b + (int64_t)h * a.s_stride_h + (int64_t)r * a.s_stride_l;
    uint32_t base = 0;
    for (int c0 = 0; c0 < a.head_dim; c0 += 64) {
        const raw x = src[c0 + lane];
        const bool pred = is_outlier(Dt<DT>::ld(x), o.thr);
        const uint64_t m = __ballot(pred);
        const uint32_t rank = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (pred && rank < cnt) {                                      // rank < cnt: never past the row's share of the pool
            o.chan[e0 + rank] = (uint8_t)(c0 + lane);
            reinterpret_cast<raw*>(o.val)[e0 + rank] = x;
        }
        base += (uint32_t)__popcll(m);
    }
}

// After dequant_kernel: the row's outliers back at their channels of dst rows [0, rows).
template <int DT>
__global__ __launch_bounds__(256) void outl_patch_kernel(const QuantArgs a, const OutlArgs o) {
    typedef typename Dt<DT>::raw raw;
    int b, h, r;
    if (!wave_item_rows(a, b, h, r)) return;
    const int lane = threadIdx.x & 63;
    const uint32_t word = o.rowinfo[(int64_t)b * o.ri_stride_b + (int64_t)h * o.ri_stride_h + a.row0 + r];
    const uint32_t cnt = word & 0xffu, start = word >> 8;
    if (cnt == 0 || (int64_t)start + cnt > o.pool_capacity) return;
    const int64_t e0 = (int64_t)b * o.pool_stride_b + start;
    raw* dst = reinterpret_cast<raw*>(a.dst) + (int64_t)b * a.s_stride_b + (int64_t)h * a.s_stride_h + (int64_t)r * a.s_stride_l;
    for (uint32_t j = lane; j < cnt; j += 64) {
        const int ch = o.chan[e0 + j];
        if (ch < a.head_dim) dst[ch] = reinterpret_cast<const raw*>(o.val)[e0 + j];
    }
}

template <int DT> __device__ __forceinline__ void widen_chunk_q(const uint4& v, float* x) {
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

// x'' of one row's lane: entries [start, start + count) of the pool (rowinfo word), channel c * EPL + e -> element e.
template <int DT, int EPL>
__device__ __forceinline__ void patch_row(float* x, uint32_t word, const uint8_t* chan, const void* val, int64_t vofs, int cap, int c) {
    typedef typename Dt<DT>::raw raw;
    const uint32_t cnt = word & 0xffu, start = word >> 8;
    if (cnt == 0 || (int64_t)start + cnt > cap) return;
    const raw* vp = reinterpret_cast<const raw*>(val) + vofs + start;
    for (uint32_t j = 0; j < cnt; ++j) {
        const int rel = (int)chan[start + j] - c * EPL;
        const float v = Dt<DT>::ld(vp[j]);
#pragma unroll
        for (int e = 0; e < EPL; ++e) x[e] = rel == e ? v : x[e];
    }
}

// grid = (b * H_q, new_rows, splits), block = 256 (4 waves) — decode_attention_kernel's mapping: LPR lanes share a row, lane c
// holds channels [c * EPL, (c + 1) * EPL) of q and acc.  Rows [0, P) are the query head's quantized prefix, [P, PQ) its KV
// head's quantized tail, [PQ, PQ + res_rows + i + 1) the residual (full precision, the step's rows included).  For a quantized row
// a lane loads its EPL codes as one word of WB = EPL * NB / 8 bytes (instead of 16 bytes), the key (scale, zero) of its channels
// from the row's key group, and the value (scale, zero) of its channel group; every load of an iteration is issued before the
// first is used.
// OUTL: each quantized row's key and value rowinfo words are loaded with the row's other loads; for a row with entries the row's
// lanes walk them (broadcast loads: every lane of the row reads the same entry) and select the entry's value into the element
// whose channel matches — a predicated select over the EPL unrolled elements, never a runtime-indexed register array.
template <int DT, int D, int NB, bool OUTL>
__global__ __launch_bounds__(256) void decode_attention_q_kernel(const DecodeQArgs a, const DecodeOArgs o) {
    typedef typename Dt<DT>::raw raw;
    constexpr int ES = Dt<DT>::esize, EPL = 16 / ES, LPR = D / EPL;
    constexpr int RPW = 64 / LPR, RPI = 4 * RPW, UNR = 4;
    constexpr int CB = D * NB / 8, WB = EPL * NB / 8, F4 = EPL / 4;
    constexpr uint32_t MASK = (1u << NB) - 1u;
    typedef typename CodeWord<WB>::type cw_t;
    __shared__ float sm_m[4 * RPW], sm_l[4 * RPW];
    __shared__ float sm_acc[4 * RPW][D];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, slot = lane / LPR, c = lane % LPR;
    const int hb = blockIdx.x, b = hb / a.n_q_heads, h = hb % a.n_q_heads, g = h / a.group;
    const int i = blockIdx.y;
    const int P = a.pre.rows, PQ = P + a.qt.rows, R = PQ + a.res_rows + i + 1;
    const int r_begin = blockIdx.z * a.rows_per_split, r_end = min(R, r_begin + a.rows_per_split);
    const int G = a.gsize, vj = (c * EPL) / G, NG = D / G;
    const float scale = a.scaling * 1.44269504088896340736f;
    float qf[EPL];
    {
        const char* qrow = reinterpret_cast<const char*>(a.q) +
            ((int64_t)b * a.q_stride_b + (int64_t)h * a.q_stride_h + (int64_t)i * a.q_stride_l) * ES;
        widen_chunk_q<DT>(reinterpret_cast<const uint4*>(qrow)[c], qf);
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
        bool valid[UNR], quant[UNR], inpre[UNR];
        uint32_t kri[UNR], vri[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int r = r0 + u * RPI + wave * RPW + slot;
            valid[u] = r < r_end;
            quant[u] = r < PQ;
            const bool pre = r < P;
            inpre[u] = pre;
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
            if constexpr (OUTL) {
                const OSegArgs& os = pre ? o.pre : o.qt;
                const int hh = pre ? h : g;
                kri[u] = lq ? os.kri[(int64_t)b * os.kri_b + (int64_t)hh * os.kri_h + rr] : 0u;
                vri[u] = lq ? os.vri[(int64_t)b * os.vri_b + (int64_t)hh * os.vri_h + rr] : 0u;
            }
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
                if constexpr (OUTL) {
                    const OSegArgs& os = inpre[u] ? o.pre : o.qt;
                    patch_row<DT, EPL>(kf, kri[u], os.kch + (int64_t)b * os.kpool_b, os.kval, (int64_t)b * os.kpool_b, os.kcap, c);
                    patch_row<DT, EPL>(vf, vri[u], os.vch + (int64_t)b * os.vpool_b, os.vval, (int64_t)b * os.vpool_b, os.vcap, c);
                }
            } else {
                widen_chunk_q<DT>(kv[u], kf);
                widen_chunk_q<DT>(vv[u], vf);
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
        } else {
            float* part = a.part + (((int64_t)hb * a.new_rows + i) * a.splits + blockIdx.z) * (D + 2);
            part[2 + tid] = o;
            if (tid == 0) { part[0] = M; part[1] = Lsum; }
        }
    }
}

static inline unsigned blocks_for(int64_t items) { return (unsigned)((items + 255) / 256); }

int launch_quantize(const QuantArgs& a, int dtype, int nbits, int mode, hipStream_t st) {
    if (a.rows <= 0) return 0;
    const int64_t items = mode == KVC_QUANT_KEYS                           // keys: 64 threads (one wave) per item
        ? (int64_t)a.bsz * a.n_heads * ((a.rows + a.group - 1) / a.group) * (a.head_dim / 64) * 64
        : (int64_t)a.bsz * a.n_heads * a.rows * (a.head_dim / a.group);
#define KVC_CASE(DT_, NB_) if (dtype == DT_ && nbits == NB_) { \
        if (mode == KVC_QUANT_KEYS) hipLaunchKernelGGL((quant_keys_kernel<DT_, NB_, false>), dim3(blocks_for(items)), dim3(256), 0, st, a, 0.0f); \
        else hipLaunchKernelGGL((quant_values_kernel<DT_, NB_, false>), dim3(blocks_for(items)), dim3(256), 0, st, a, 0.0f); return 0; }
    KVC_CASE(KVC_BF16, 2) KVC_CASE(KVC_BF16, 4) KVC_CASE(KVC_BF16, 8) KVC_CASE(KVC_FP16, 2) KVC_CASE(KVC_FP16, 4) KVC_CASE(KVC_FP16, 8)
    KVC_CASE(KVC_FP32, 2) KVC_CASE(KVC_FP32, 4) KVC_CASE(KVC_FP32, 8)
#undef KVC_CASE
    return KVC_ERR_UNSUPPORTED;
}

int launch_dequantize(const QuantArgs& a, int dtype, int nbits, int mode, hipStream_t st) {
    if (a.rows <= 0) return 0;
    const int64_t items = (int64_t)a.bsz * a.n_heads * a.rows * (a.head_dim * nbits / 32);
#define KVC_CASE(DT_, NB_) if (dtype == DT_ && nbits == NB_) { \
        if (mode == KVC_QUANT_KEYS) hipLaunchKernelGGL((dequant_kernel<DT_, NB_, KVC_QUANT_KEYS>), dim3(blocks_for(items)), dim3(256), 0, st, a); \
        else hipLaunchKernelGGL((dequant_kernel<DT_, NB_, KVC_QUANT_VALUES>), dim3(blocks_for(items)), dim3(256), 0, st, a); return 0; }
    KVC_CASE(KVC_BF16, 2) KVC_CASE(KVC_BF16, 4) KVC_CASE(KVC_BF16, 8) KVC_CASE(KVC_FP16, 2) KVC_CASE(KVC_FP16, 4) KVC_CASE(KVC_FP16, 8)
    KVC_CASE(KVC_FP32, 2) KVC_CASE(KVC_FP32, 4) KVC_CASE(KVC_FP32, 8)
#undef KVC_CASE
    return KVC_ERR_UNSUPPORTED;
}

// `append` carries the residual as decode_append_kernel's tail and, for decode_combine_kernel, the output and the splits.
int launch_decode_step_quant(DecodeQArgs a, int dtype, int head_dim, int nbits, const DecodeArgs& append, hipStream_t st) {
    launch_decode_append(append, st);
    const int rows = a.pre.rows + a.qt.rows + a.res_rows + a.new_rows;
    if (a.splits < 1 || a.part == nullptr) a.splits = 1;
    a.rows_per_split = a.splits == 1 ? rows : ((rows + a.splits - 1) / a.splits + 63) / 64 * 64;
    if (a.splits > 1) a.splits = (rows + a.rows_per_split - 1) / a.rows_per_split;          // no empty split
    const dim3 grid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows, (unsigned)a.splits);
    int rc = KVC_ERR_UNSUPPORTED;
#define KVC_CASE(DT_, D_, NB_) if (dtype == DT_ && head_dim == D_ && nbits == NB_) { \
        hipLaunchKernelGGL((decode_attention_q_kernel<DT_, D_, NB_, false>), grid, dim3(256), 0, st, a, DecodeOArgs{}); rc = 0; }
    KVC_CASE(KVC_BF16, 128, 2) KVC_CASE(KVC_BF16, 128, 4) KVC_CASE(KVC_BF16, 128, 8)
    KVC_CASE(KVC_BF16, 64, 2) KVC_CASE(KVC_BF16, 64, 4) KVC_CASE(KVC_BF16, 64, 8)
    KVC_CASE(KVC_FP16, 128, 2) KVC_CASE(KVC_FP16, 128, 4) KVC_CASE(KVC_FP16, 128, 8)
    KVC_CASE(KVC_FP16, 64, 2) KVC_CASE(KVC_FP16, 64, 4) KVC_CASE(KVC_FP16, 64, 8)
    KVC_CASE(KVC_FP32, 128, 2) KVC_CASE(KVC_FP32, 128, 4) KVC_CASE(KVC_FP32, 128, 8)
    KVC_CASE(KVC_FP32, 64, 2) KVC_CASE(KVC_FP32, 64, 4) KVC_CASE(KVC_FP32, 64, 8)
#undef KVC_CASE
    if (rc) return rc;
    if (a.splits > 1) {
        DecodeArgs cmb = append;
        cmb.part = a.part; cmb.splits = a.splits;
        return launch_decode_combine(cmb, dtype, head_dim, st);
    }
    return 0;
}

int launch_quantize_outliers(const QuantArgs& a, const OutlArgs& o, int dtype, int nbits, int mode, hipStream_t st) {
    if (a.rows <= 0) return 0;
    const int64_t items = mode == KVC_QUANT_KEYS
        ? (int64_t)a.bsz * a.n_heads * ((a.rows + a.group - 1) / a.group) * (a.head_dim / 64) * 64
        : (int64_t)a.bsz * a.n_heads * a.rows * (a.head_dim / a.group);
    const unsigned row_waves = blocks_for((int64_t)a.bsz * a.n_heads * a.rows * 64);
    int rc = KVC_ERR_UNSUPPORTED;
#define KVC_CASE(DT_, NB_) if (dtype == DT_ && nbits == NB_) { \
        if (mode == KVC_QUANT_KEYS) hipLaunchKernelGGL((quant_keys_kernel<DT_, NB_, true>), dim3(blocks_for(items)), dim3(256), 0, st, a, o.thr); \
        else hipLaunchKernelGGL((quant_values_kernel<DT_, NB_, true>), dim3(blocks_for(items)), dim3(256), 0, st, a, o.thr); \
        hipLaunchKernelGGL((outl_count_kernel<DT_>), dim3(row_waves), dim3(256), 0, st, a, o); \
        hipLaunchKernelGGL(outl_scan_kernel, dim3((unsigned)a.bsz), dim3(1024), 0, st, a, o); \
        hipLaunchKernelGGL((outl_write_kernel<DT_>), dim3(row_waves), dim3(256), 0, st, a, o); rc = 0; }
    KVC_CASE(KVC_BF16, 2) KVC_CASE(KVC_BF16, 4) KVC_CASE(KVC_BF16, 8) KVC_CASE(KVC_FP16, 2) KVC_CASE(KVC_FP16, 4) KVC_CASE(KVC_FP16, 8)
    KVC_CASE(KVC_FP32, 2) KVC_CASE(KVC_FP32, 4) KVC_CASE(KVC_FP32, 8)
#undef KVC_CASE
    return rc;
}

int launch_dequantize_outliers(const QuantArgs& a, const OutlArgs& o, int dtype, int nbits, int mode, hipStream_t st) {
    if (a.rows <= 0) return 0;
    if (int rc = launch_dequantize(a, dtype, nbits, mode, st)) return rc;
    const unsigned row_waves = blocks_for((int64_t)a.bsz * a.n_heads * a.rows * 64);
    if (dtype == KVC_BF16) hipLaunchKernelGGL((outl_patch_kernel<KVC_BF16>), dim3(row_waves), dim3(256), 0, st, a, o);
    else if (dtype == KVC_FP16) hipLaunchKernelGGL((outl_patch_kernel<KVC_FP16>), dim3(row_waves), dim3(256), 0, st, a, o);
    else hipLaunchKernelGGL((outl_patch_kernel<KVC_FP32>), dim3(row_waves), dim3(256), 0, st, a, o);
    return 0;
}

int launch_decode_step_quant_outliers(DecodeQArgs a, const DecodeOArgs& o, int dtype, int head_dim, int nbits, const DecodeArgs& append,
                                      hipStream_t st) {
    launch_decode_append(append, st);
    const int rows = a.pre.rows + a.qt.rows + a.res_rows + a.new_rows;
    if (a.splits < 1 || a.part == nullptr) a.splits = 1;
    a.rows_per_split = a.splits == 1 ? rows : ((rows + a.splits - 1) / a.splits + 63) / 64 * 64;
    if (a.splits > 1) a.splits = (rows + a.rows_per_split - 1) / a.rows_per_split;          // the same splits as the KIVI step
    const dim3 grid((unsigned)(a.bsz * a.n_q_heads), (unsigned)a.new_rows, (unsigned)a.splits);
    int rc = KVC_ERR_UNSUPPORTED;
#define KVC_CASE(DT_, D_, NB_) if (dtype == DT_ && head_dim == D_ && nbits == NB_) { \
        hipLaunchKernelGGL((decode_attention_q_kernel<DT_, D_, NB_, true>), grid, dim3(256), 0, st, a, o); rc = 0; }
    KVC_CASE(KVC_BF16, 128, 2) KVC_CASE(KVC_BF16, 128, 4) KVC_CASE(KVC_BF16, 128, 8)
    KVC_CASE(KVC_BF16, 64, 2) KVC_CASE(KVC_BF16, 64, 4) KVC_CASE(KVC_BF16, 64, 8)
    KVC_CASE(KVC_FP16, 128, 2) KVC_CASE(KVC_FP16, 128, 4) KVC_CASE(KVC_FP16, 128, 8)
    KVC_CASE(KVC_FP16, 64, 2) KVC_CASE(KVC_FP16, 64, 4) KVC_CASE(KVC_FP16, 64, 8)
    KVC_CASE(KVC_FP32, 128, 2) KVC_CASE(KVC_FP32, 128, 4) KVC_CASE(KVC_FP32, 128, 8)
    KVC_CASE(KVC_FP32, 64, 2) KVC_CASE(KVC_FP32, 64, 4) KVC_CASE(KVC_FP32, 64, 8)
#undef KVC_CASE
    if (rc) return rc;
    if (a.splits > 1) {
        DecodeArgs cmb = append;
        cmb.part = a.part; cmb.splits = a.splits;
        return launch_decode_combine(cmb, dtype, head_dim, st);
    }
    return 0;
}

}  // namespace kvc
