"""numpy restatement of the quantized decode cache (include/kvc.h): the KIVI-style rounding rule, the packing of the codes, the
metadata layout, de-quantization and fp32 attention over the de-quantized cache.  Test infrastructure, like cpu_compress.py:
the GPU tests compare the HIP kernels against it, the CPU tests monkeypatch the `_kvc` quant entry points with the torch-facing
stand-ins at the bottom (quantize_rows, dequantize_rows, decode_step_quant) so the cache layer runs without a GPU."""
import numpy as np
import torch

KEYS, VALUES = 0, 1


def _f32(x):
    return x.float().cpu().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float32)


def _codes(x, mn, sc, nbits):
    """code = scale > 0 ? clamp(rint((x - mn) / scale), 0, qmax) : 0 — all in fp32 (numpy float32 ops are IEEE-rounded)."""
    qmax = np.float32(2 ** nbits - 1)
    pos = sc > 0
    c = np.rint((x - mn) / np.where(pos, sc, np.float32(1)))
    return np.where(pos, np.clip(c, 0, qmax), 0).astype(np.uint8)


def quantize(x, mode, nbits, group_size):
    """x [..., rows, D] float32 -> (codes [..., rows, D] uint8 unpacked, scale, zero).
    KEYS: scale / zero [..., ceil(rows / G), D] (per channel over G rows; a partial last group has its own min / max);
    VALUES: scale / zero [..., rows, D / G] (per row over G channels)."""
    x = np.asarray(x, dtype=np.float32)
    qmax = np.float32(2 ** nbits - 1)
    G = group_size
    if mode == KEYS:
        rows = x.shape[-2]
        ng = -(-rows // G)
        codes = np.empty(x.shape, dtype=np.uint8)
        sc = np.empty(x.shape[:-2] + (ng, x.shape[-1]), dtype=np.float32)
        zp = np.empty_like(sc)
        for g in range(ng):
            blk = x[..., g * G:(g + 1) * G, :]
            mn, mx = blk.min(axis=-2), blk.max(axis=-2)
            s = (mx - mn) / qmax
            sc[..., g, :], zp[..., g, :] = s, mn
            codes[..., g * G:(g + 1) * G, :] = _codes(blk, mn[..., None, :], s[..., None, :], nbits)
        return codes, sc, zp
    D = x.shape[-1]
    xg = x.reshape(x.shape[:-1] + (D // G, G))
    mn, mx = xg.min(axis=-1), xg.max(axis=-1)
    s = (mx - mn) / qmax
    codes = _codes(xg, mn[..., None], s[..., None], nbits).reshape(x.shape)
    return codes, s.astype(np.float32), mn.astype(np.float32)


def pack(codes, nbits):
    """[..., D] codes -> [..., D * nbits / 8] bytes: channel d at bit d * nbits of the row, little-endian within each byte."""
    per = 8 // nbits
    c = codes.astype(np.uint32).reshape(codes.shape[:-1] + (codes.shape[-1] // per, per))
    out = np.zeros(c.shape[:-1], dtype=np.uint32)
    for e in range(per):
        out |= c[..., e] << (e * nbits)
    return out.astype(np.uint8)


def unpack(packed, nbits):
    per = 8 // nbits
    p = np.asarray(packed, dtype=np.uint8).astype(np.uint32)
    out = np.stack([(p >> (e * nbits)) & (2 ** nbits - 1) for e in range(per)], axis=-1)
    return out.reshape(p.shape[:-1] + (p.shape[-1] * per,)).astype(np.uint8)


def meta_array(sc, zp, mode):
    """The metadata layout of kvc.h: KEYS [..., groups, 2, D] (scales, then zeros); VALUES [..., rows, D / G, 2] (scale, zero)."""
    return np.stack([sc, zp], axis=-2 if mode == KEYS else -1).astype(np.float32)


def split_meta(meta, mode):
    meta = np.asarray(meta, dtype=np.float32)
    return (meta[..., 0, :], meta[..., 1, :]) if mode == KEYS else (meta[..., 0], meta[..., 1])


def dequantize(codes, sc, zp, mode, group_size, row0=0):
    """x' = code * scale + zero, rounded through float64 (kvc.h's fmaf up to a double rounding: within 1 ulp of fp32).
    codes [..., rows, D] unpacked; KEYS: the rows' group is (row0 + r) / G; VALUES: sc / zp [..., rows, D / G]."""
    c = codes.astype(np.float64)
    rows = codes.shape[-2]
    if mode == KEYS:
        gi = (row0 + np.arange(rows)) // group_size
        s, z = sc[..., gi, :], zp[..., gi, :]
    else:
        s, z = np.repeat(sc, group_size, axis=-1), np.repeat(zp, group_size, axis=-1)
    return (c * s.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def roundtrip(x, mode, nbits, group_size):
    """The de-quantized values the cache holds for x [..., rows, D] (fp32)."""
    c, s, z = quantize(_f32(x), mode, nbits, group_size)
    return dequantize(c, s, z, mode, group_size)


def attention(q, K, V, scaling, causal_new=0):
    """fp32 softmax(q K^T * scaling) V; q [b, H, t, D], K / V [b, H, n, D] (already H-expanded); token i of the t new ones sees
    the first n - t + i + 1 rows when causal_new = t."""
    q, K, V = (_f32(x).astype(np.float64) for x in (q, K, V))
    s = q @ np.swapaxes(K, -1, -2) * scaling
    t, n = q.shape[-2], K.shape[-2]
    if causal_new:
        for i in range(t):
            s[..., i, n - t + i + 1:] = -np.inf
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return (p @ V).astype(np.float32)


# ---- torch-facing stand-ins with the signatures of kvcache_factory_amd._kvc (CPU tensors) ------------------------------------
def quantize_rows(src, codes, meta, row0, mode, nbits, group_size):
    x = _f32(src)
    c, s, z = quantize(x, mode, nbits, group_size)
    n = x.shape[-2]
    codes[:, :, row0:row0 + n] = torch.from_numpy(pack(c, nbits))
    m = torch.from_numpy(meta_array(s, z, mode))
    if mode == KEYS:
        g0 = row0 // group_size
        meta[:, :, g0:g0 + m.shape[2]] = m
    else:
        meta[:, :, row0:row0 + n] = m


def dequantize_rows(codes, meta, row0, rows, mode, nbits, group_size, dtype):
    c = unpack(codes[:, :, row0:row0 + rows].cpu().numpy(), nbits)
    s, z = split_meta(meta.cpu().numpy(), mode)
    if mode == VALUES:
        s, z = s[:, :, row0:row0 + rows], z[:, :, row0:row0 + rows]
    return torch.from_numpy(dequantize(c, s, z, mode, group_size, row0)).to(dtype)


def segment_values(seg, nbits, group_size, dtype=torch.float32):
    """(k_codes, v_codes, k_meta, v_meta, rows) -> de-quantized (K, V) [b, H, rows, D]."""
    kc, vc, km, vm, rows = seg
    return (dequantize_rows(kc.cpu(), km.cpu(), 0, rows, KEYS, nbits, group_size, dtype),
            dequantize_rows(vc.cpu(), vm.cpu(), 0, rows, VALUES, nbits, group_size, dtype))


def decode_step_quant(q, k_new, v_new, prefix, qtail, k_res, v_res, res_rows, scaling, nbits, group_size, residual_length):
    """What kvc_decode_step_quant computes, in fp32 over the de-quantized segments: appends the step's rows to the residual."""
    b, hq, t, D = q.shape
    hkv = k_new.shape[1]
    k_res[:, :, res_rows:res_rows + t] = k_new
    v_res[:, :, res_rows:res_rows + t] = v_new
    Ks, Vs = [], []
    for seg, heads in ((prefix, hq), (qtail, hkv)):
        if seg is not None and seg[4] > 0:
            k, v = segment_values(seg, nbits, group_size)
            Ks.append(k.repeat_interleave(hq // heads, 1))
            Vs.append(v.repeat_interleave(hq // heads, 1))
    Ks.append(k_res[:, :, :res_rows + t].float().repeat_interleave(hq // hkv, 1))
    Vs.append(v_res[:, :, :res_rows + t].float().repeat_interleave(hq // hkv, 1))
    out = attention(q, torch.cat(Ks, 2), torch.cat(Vs, 2), scaling, causal_new=t)
    return torch.from_numpy(out).to(q.dtype).transpose(1, 2).contiguous()
