"""numpy restatement of the quantized cache with exact outliers (include/kvc.h, "quantized cache with exact outliers"): the split,
the dense codes (quant_ref's KIVI rule on the split input), the outlier pool's bytes, de-quantization and the attention.  Test
infrastructure: the GPU tests compare the HIP kernels against it, the CPU tests monkeypatch the `_kvc` outlier entry points with the
torch-facing stand-ins at the bottom so KVQuantCompressedLayer runs without a GPU."""
import numpy as np
import torch

import quant_ref as Q

KEYS, VALUES = Q.KEYS, Q.VALUES


def round_threshold(threshold, dtype):
    """T': the threshold rounded to nearest even in the cache dtype (fp16 range overflow -> inf); fp32 keeps the fp32 value."""
    t = np.float32(threshold)
    if dtype == torch.float16:
        return np.float32(np.float16(t))
    if dtype == torch.bfloat16:
        u = int(t.view(np.uint32))
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return np.array([u], dtype=np.uint32).view(np.float32)[0]
    return t


def split(x, thr):
    """(outlier mask, dense input): x is an outlier iff x < -T' or x > T' (+-inf are, NaN is not); the dense input has +0 there."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        mask = (x < -thr) | (x > thr)
    return mask, np.where(mask, np.float32(0.0), x).astype(np.float32)


def quantize(x, mode, nbits, group_size, thr):
    """(codes, scale, zero) of the dense input, as quant_ref.quantize, and the outlier mask."""
    mask, dense = split(x, thr)
    c, s, z = Q.quantize(dense, mode, nbits, group_size)
    return c, s, z, mask


def pool_layout(x, mask, used, pool_capacity, row0=0, capacity=None):
    """The pool a quantize call leaves for x [b, H, rows, D] (widened values) with `mask`, starting at used[b]:
    returns (entries: list per b of (chan, val) in (h, row, channel) order with their positions, new used [b],
    rowinfo [b, H, row0 + rows] uint32 of the call's rows (rows before row0 zero)).  Entries of rows that do not fit wholly below
    pool_capacity are not written and their rowinfo is 0; used still advances by every outlier found."""
    b, H, rows, D = x.shape
    ri = np.zeros((b, H, (capacity or row0 + rows)), dtype=np.uint32)
    used = np.asarray(used, dtype=np.int64).copy()
    writes = []
    for bi in range(b):
        w = []
        pos = int(used[bi])
        for h in range(H):
            for r in range(rows):
                ch = np.nonzero(mask[bi, h, r])[0]
                n = len(ch)
                if n and pos + n <= pool_capacity:
                    ri[bi, h, row0 + r] = (pos << 8) | n
                    w.extend((pos + j, int(c), x[bi, h, r, c]) for j, c in enumerate(ch))
                pos += n
        used[bi] = min(pos, 2 ** 31 - 1)
        writes.append(w)
    return writes, used.astype(np.int32), ri


def dequantize(codes, sc, zp, mask, x, mode, group_size, row0=0):
    """x'' = x at an outlier, otherwise quant_ref.dequantize's x'."""
    d = Q.dequantize(codes, sc, zp, mode, group_size, row0)
    return np.where(mask, np.asarray(x, dtype=np.float32), d).astype(np.float32)


def roundtrip(x, mode, nbits, group_size, thr):
    xf = Q._f32(x)
    c, s, z, m = quantize(xf, mode, nbits, group_size, thr)
    return dequantize(c, s, z, m, xf, mode, group_size)


# ---- torch-facing stand-ins with the signatures of kvcache_factory_amd._kvc (CPU tensors) ------------------------------------
def quantize_rows_outliers(src, codes, meta, pool, row0, mode, nbits, group_size, threshold):
    chan, val, used, ri = pool
    thr = round_threshold(threshold, src.dtype)
    x = Q._f32(src)
    mask, dense = split(x, thr)
    Q.quantize_rows(torch.from_numpy(dense), codes, meta, row0, mode, nbits, group_size)
    writes, new_used, ri_new = pool_layout(x, mask, used.numpy(), chan.shape[1], row0, ri.shape[2])
    n = x.shape[2]
    ri[:, :, row0:row0 + n] = torch.from_numpy(ri_new[:, :, row0:row0 + n].view(np.int32))
    for bi, w in enumerate(writes):
        for pos, c, v in w:
            chan[bi, pos] = c
            val[bi, pos] = float(v)
    used.copy_(torch.from_numpy(new_used))


def patch(out, pool, row0, rows):
    """Write the pool's outliers of segment rows [row0, row0 + rows) into out [b, H, rows, D]."""
    chan, val, _, ri = pool
    w = ri[:, :, row0:row0 + rows].numpy().view(np.uint32)
    for bi, h, r in zip(*np.nonzero(w & 0xFF)):
        start, cnt = int(w[bi, h, r] >> 8), int(w[bi, h, r] & 0xFF)
        for j in range(start, start + cnt):
            out[bi, h, r, int(chan[bi, j])] = val[bi, j]
    return out


def dequantize_rows_outliers(codes, meta, pool, row0, rows, mode, nbits, group_size, dtype):
    return patch(Q.dequantize_rows(codes, meta, row0, rows, mode, nbits, group_size, dtype), pool, row0, rows)


def segment_values(seg, pools, nbits, group_size, dtype=torch.float32):
    kc, vc, km, vm, rows = seg
    return (dequantize_rows_outliers(kc.cpu(), km.cpu(), tuple(t.cpu() for t in pools[0]), 0, rows, KEYS, nbits, group_size, dtype),
            dequantize_rows_outliers(vc.cpu(), vm.cpu(), tuple(t.cpu() for t in pools[1]), 0, rows, VALUES, nbits, group_size, dtype))


def decode_step_quant_outliers(q, k_new, v_new, prefix, qtail, prefix_outl, qtail_outl, k_res, v_res, res_rows, scaling, nbits, group_size,
                               residual_length):
    """What kvc_decode_step_quant_outliers computes, in fp32 over the de-quantized segments (outliers exact)."""
    b, hq, t, D = q.shape
    hkv = k_new.shape[1]
    k_res[:, :, res_rows:res_rows + t] = k_new
    v_res[:, :, res_rows:res_rows + t] = v_new
    Ks, Vs = [], []
    for seg, pools, heads in ((prefix, prefix_outl, hq), (qtail, qtail_outl, hkv)):
        if seg is not None and seg[4] > 0:
            k, v = segment_values(seg, pools, nbits, group_size)
            Ks.append(k.repeat_interleave(hq // heads, 1))
            Vs.append(v.repeat_interleave(hq // heads, 1))
    Ks.append(k_res[:, :, :res_rows + t].float().cpu().repeat_interleave(hq // hkv, 1))
    Vs.append(v_res[:, :, :res_rows + t].float().cpu().repeat_interleave(hq // hkv, 1))
    out = Q.attention(q, torch.cat(Ks, 2), torch.cat(Vs, 2), scaling, causal_new=t)
    return torch.from_numpy(out).to(q.dtype).transpose(1, 2).contiguous().to(q.device)
