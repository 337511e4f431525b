// kvc_decode_compress.hip — decode-stage compression of the SPLIT decode cache (include/kvc.h: kvc_decode_compress).
// The cache of one layer is a prefix per QUERY head and a tail per KV head; the virtual key row r of query head h is
// prefix[h][r] for r < P and tail[h / G][r - P] otherwise.  Two kernels read that two-part cache where it lies:
//   dc_scan_kernel   : the window logits [h][L][W] and per-partition row maxima [h][n_parts][W] in the ScoreArgs workspace
//                      layout, so that kvc_score.hip's softmax / pooling stage runs on them unchanged (stage mask 6);
//   dc_gather_kernel : cat(K[idx], K[L-W:L]) and the same for V, each kept row fetched from the segment that holds it.
// Arithmetic of a logit (kvc_score.hip logits_kernel, the oracle's KVCO_DOT_CHAIN): the d-ascending fp32 fmaf chain from +0,
// rounded to dtype, divided by sqrt(D) (correctly rounded) and rounded again, and on the last W keys the local causal mask
// (+ finfo.min, rounded).  Here the chain runs on the VALU: a decode cache is scored by W (8 .. 64) query rows per query
// head, too few to fill the 32-row tile of the f32-input MFMA once a query head's prefix is its own key set.
#include "kvc_common.h"
#include "kvc_launch.h"

namespace kvc {

constexpr int DC_THREADS = 256;

// One thread per key row: the row's 16-byte chunks are widened once and contracted against WB query rows held in LDS as
// fp32 (every lane reads the same address: broadcast).  WV = W for the built windows 8 / 16 / 32 / 64 (one pass, W known at
// compile time); WV = 0 otherwise: ceil(W / 8) passes of 8 rows over the same keys, the image padded with zero rows.
template <int DT, int D, int WV>
__global__ __launch_bounds__(DC_THREADS) void dc_scan_kernel(const DcScanArgs a) {
    constexpr int WB = WV > 0 ? WV : 8;           // query rows per pass
    typedef typename Dt<DT>::raw raw;
    constexpr int ES = Dt<DT>::esize;
    constexpr int EPC = 16 / ES;                  // elements per 16-byte chunk
    constexpr int CH = D / EPC;                   // chunks per row
    extern __shared__ __attribute__((aligned(16))) float qs[];     // [passes * WB][D] fp32
    __shared__ float red[DC_THREADS / 64][WB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hb = blockIdx.y, part = blockIdx.x;
    const int hq = hb % a.n_q_heads, b = hb / a.n_q_heads;
    const int W = WV > 0 ? WV : a.window, L = a.q_len, P = a.prefix_rows;
    const int rows_img = (W + WB - 1) / WB * WB;

    // query image: window row w = ring row (ring_start + w) % W, widened exactly; padded rows are zero
    const raw* ring = reinterpret_cast<const raw*>(a.ring) + (int64_t)b * a.ring_sb + (int64_t)hq * a.ring_sh;
    for (int i = tid; i < rows_img * D; i += DC_THREADS) {
        const int w = i / D, d = i % D;
        float x = 0.0f;
        if (w < W) {
            int rr = a.ring_start + w;
            rr = rr >= W ? rr - W : rr;
            x = Dt<DT>::ld(ring[(int64_t)rr * D + d]);
        }
        qs[i] = x;
    }
    __syncthreads();

    const raw* kp = reinterpret_cast<const raw*>(a.kp) + (int64_t)b * a.kp_sb + (int64_t)hq * a.kp_sh;
    const raw* kt = reinterpret_cast<const raw*>(a.kt) + (int64_t)b * a.kt_sb + (int64_t)(hq / a.group) * a.kt_sh;
    raw* lg = reinterpret_cast<raw*>(a.logits) + (int64_t)hb * L * W;
    const int k0 = part * a.keys_per_part;
    const int k1 = k0 + a.keys_per_part < L ? k0 + a.keys_per_part : L;
    const bool vec_rows = ((W * ES) & 15) == 0;  // a key's W logits start 16-byte aligned

    for (int w0 = 0; w0 < W; w0 += WB) {
        float mx[WB];
#pragma unroll
        for (int e = 0; e < WB; ++e) mx[e] = -__builtin_inff();
        for (int key = k0 + tid; key < k1; key += DC_THREADS) {
            const uint4* krow = reinterpret_cast<const uint4*>(key < P ? kp + (int64_t)key * D : kt + (int64_t)(key - P) * D);
            float acc[WB];
#pragma unroll
            for (int e = 0; e < WB; ++e) acc[e] = 0.0f;
#pragma unroll 1
            for (int c = 0; c < CH; ++c) {
                const uint4 v = krow[c];
                const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
                float kf[EPC];
#pragma unroll
                for (int x = 0; x < EPC; ++x) {
                    if constexpr (ES == 4) kf[x] = u2f(wd[x]);
                    else kf[x] = Dt<DT>::ld((raw)((wd[x >> 1] >> ((x & 1) * 16)) & 0xffffu));
                }
#pragma unroll
                for (int e = 0; e < WB; ++e) {
                    const float4* qv = reinterpret_cast<const float4*>(qs + (w0 + e) * D + c * EPC);
#pragma unroll
                    for (int x4 = 0; x4 < EPC / 4; ++x4) {
                        const float4 q4 = qv[x4];
                        acc[e] = __builtin_fmaf(q4.x, kf[4 * x4 + 0], acc[e]);
                        acc[e] = __builtin_fmaf(q4.y, kf[4 * x4 + 1], acc[e]);
                        acc[e] = __builtin_fmaf(q4.z, kf[4 * x4 + 2], acc[e]);
                        acc[e] = __builtin_fmaf(q4.w, kf[4 * x4 + 3], acc[e]);
                    }
                }
            }
            // the three roundings and the local causal mask of logits_kernel's epilogue
            float x[WB];
#pragma unroll
            for (int e = 0; e < WB; ++e) {
                const int w = w0 + e;
                float v = rnd<DT>(acc[e]);
                v = rnd<DT>(v / a.sqrt_d);
                if (key >= L - W && (key - (L - W)) > w) v = rnd<DT>(v + Dt<DT>::finfo_min());
                x[e] = v;
                if (w < W) mx[e] = v > mx[e] ? v : mx[e];
            }
            raw* dst = lg + (int64_t)key * W + w0;
            if (vec_rows && w0 + WB <= W) {
                if constexpr (ES == 2) {
#pragma unroll
                    for (int e = 0; e < WB; e += 8) {
                        uint4 pk;
                        pk.x = (uint32_t)Dt<DT>::st(x[e + 0]) | ((uint32_t)Dt<DT>::st(x[e + 1]) << 16);
                        pk.y = (uint32_t)Dt<DT>::st(x[e + 2]) | ((uint32_t)Dt<DT>::st(x[e + 3]) << 16);
                        pk.z = (uint32_t)Dt<DT>::st(x[e + 4]) | ((uint32_t)Dt<DT>::st(x[e + 5]) << 16);
                        pk.w = (uint32_t)Dt<DT>::st(x[e + 6]) | ((uint32_t)Dt<DT>::st(x[e + 7]) << 16);
                        *reinterpret_cast<uint4*>(dst + e) = pk;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < WB; e += 4) *reinterpret_cast<float4*>(dst + e) = make_float4(x[e], x[e + 1], x[e + 2], x[e + 3]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < WB; ++e)
                    if (w0 + e < W) dst[e] = Dt<DT>::st(x[e]);
            }
        }
        // row maxima of this partition: wave fold, then across the block's waves
#pragma unroll
        for (int e = 0; e < WB; ++e) {
            float m = mx[e];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const float o = __shfl_xor(m, s, 64);
                m = o > m ? o : m;
            }
            if (lane == 0) red[wave][e] = m;
        }
        __syncthreads();
        if (tid < WB && w0 + tid < W) {
            float m = red[0][tid];
#pragma unroll
            for (int wv = 1; wv < DC_THREADS / 64; ++wv) { const float o = red[wv][tid]; m = o > m ? o : m; }
            a.pmax[((int64_t)hb * a.n_parts + part) * W + w0 + tid] = m;
        }
        __syncthreads();
    }
}

// A8 over the two segments: output row t < k is virtual row idx[t] (t without idx), rows k .. k+W-1 are L-W .. L-1; virtual
// row r < P is prefix row r of the query head, else tail row r - P of its KV head.  K and V by blockIdx.z, 16 bytes a lane.
__global__ __launch_bounds__(256) void dc_gather_kernel(const DcGatherArgs a) {
    const int which = blockIdx.z;
    const int lanes_per_row = a.row_bytes >> 4;
    const int rows_per_block = 256 / lanes_per_row;
    const int r = threadIdx.x / lanes_per_row, c = threadIdx.x % lanes_per_row;
    const int cap = a.k + a.window;
    const int t = blockIdx.x * rows_per_block + r;
    if (r >= rows_per_block || t >= cap) return;
    const int hb = blockIdx.y, b = hb / a.n_q_heads, h = hb % a.n_q_heads;
    const int D = a.row_bytes / a.esize;
    int64_t srow;
    if (t < a.k) srow = a.idx ? a.idx[(int64_t)hb * a.k + t] : (int64_t)t;
    else srow = (int64_t)(a.q_len - a.window) + (t - a.k);
    const char* src;
    if (srow < a.prefix_rows)
        src = reinterpret_cast<const char*>(a.src_p[which]) + ((int64_t)b * a.p_sb + (int64_t)h * a.p_sh + srow * D) * a.esize;
    else
        src = reinterpret_cast<const char*>(a.src_t[which]) +
              ((int64_t)b * a.t_sb + (int64_t)(h / a.group) * a.t_sh + (srow - a.prefix_rows) * D) * a.esize;
    char* dst = reinterpret_cast<char*>(a.out[which]) + ((int64_t)b * a.o_sb + (int64_t)h * a.o_sh + (int64_t)t * D) * a.esize;
    *reinterpret_cast<uint4*>(dst + c * 16) = *reinterpret_cast<const uint4*>(src + c * 16);
}

template <int DT, int D, int WV>
static void launch_dc_scan_t(const DcScanArgs& a, int bsz, hipStream_t st) {
    constexpr int WB = WV > 0 ? WV : 8;
    const size_t lds = (size_t)((a.window + WB - 1) / WB * WB) * D * sizeof(float);
    dim3 grid((unsigned)a.n_parts, (unsigned)(bsz * a.n_q_heads));
    hipLaunchKernelGGL((dc_scan_kernel<DT, D, WV>), grid, dim3(DC_THREADS), lds, st, a);
}

template <int DT, int D>
static void launch_dc_scan_w(const DcScanArgs& a, int bsz, hipStream_t st) {
    switch (a.window) {
        case 8:  launch_dc_scan_t<DT, D, 8>(a, bsz, st); break;
        case 16: launch_dc_scan_t<DT, D, 16>(a, bsz, st); break;
        case 32: launch_dc_scan_t<DT, D, 32>(a, bsz, st); break;
        case 64: launch_dc_scan_t<DT, D, 64>(a, bsz, st); break;
        default: launch_dc_scan_t<DT, D, 0>(a, bsz, st); break;
    }
}

int launch_dc_scan(const DcScanArgs& a, int dtype, int head_dim, int bsz, hipStream_t st) {
#define KVC_CASE(DT_, D_) if (dtype == DT_ && head_dim == D_) { launch_dc_scan_w<DT_, D_>(a, bsz, st); return 0; }
    KVC_CASE(KVC_BF16, 128); KVC_CASE(KVC_BF16, 64);
    KVC_CASE(KVC_FP16, 128); KVC_CASE(KVC_FP16, 64);
    KVC_CASE(KVC_FP32, 128); KVC_CASE(KVC_FP32, 64);
#undef KVC_CASE
    return KVC_ERR_UNSUPPORTED;
}

int launch_dc_gather(const DcGatherArgs& a, int bsz, hipStream_t st) {
    const int lanes_per_row = a.row_bytes / 16;
    const int rows_per_block = 256 / lanes_per_row;
    const int cap = a.k + a.window;
    dim3 grid((unsigned)((cap + rows_per_block - 1) / rows_per_block), (unsigned)(bsz * a.n_q_heads), 2u);
    hipLaunchKernelGGL(dc_gather_kernel, grid, dim3(256), 0, st, a);
    return 0;
}

}  // namespace kvc
