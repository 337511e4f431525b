"""The quantized cache with exact outliers without a GPU: the split rule against torch's own comparison, the numpy restatement
(tests/kvquant_ref.py) against the reference's semantics restated in torch, the pool layout, C-ABI validation of the new entry
points, the cache's arguments, AdaKV / HeadKV / ThinK refusing it, and KVQuantCompressedLayer's bookkeeping with the `_kvc` entry
points replaced by the restatement (flush, pool growth, beams, fullkv, host read-backs)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kvquant_ref as KQ
import quant_ref as Q
from kvcache_factory_amd import _kvc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the split rule -----------------------------------------------------------------------------------------------------------
def _torch_mask(x, T):
    return ((x < -T) | (x > T)).numpy()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("T", [6.1, 6.0, 0.3, 1000.0])
def test_split_rule_matches_torch(dtype, T):
    """T' is T rounded to dtype; +-T' are not outliers, the next representable values beyond are; +-inf are, NaN is not."""
    thr = KQ.round_threshold(T, dtype)
    assert float(torch.tensor(T, dtype=dtype)) == float(thr) or dtype == torch.float32
    edge = torch.tensor([thr, -thr], dtype=torch.float32).to(dtype)
    beyond = torch.nextafter(edge.float(), torch.tensor([np.inf, -np.inf])).to(dtype)
    if dtype != torch.float32:                                   # the next value of the 16-bit type, not of fp32
        step = torch.tensor([1, -1], dtype=torch.int16)
        beyond = (edge.view(torch.int16) + torch.where(edge > 0, step, -step).abs()).view(dtype)
    x = torch.cat([edge, beyond, torch.tensor([np.inf, -np.inf, np.nan, 0.0, -0.0], dtype=dtype),
                   torch.randn(200, generator=torch.Generator().manual_seed(1)).to(dtype) * T])
    got, _ = KQ.split(x.float().numpy(), thr)
    assert np.array_equal(got, _torch_mask(x, T)), (dtype, T)
    assert not got[0] and not got[1] and got[2] and got[3] and got[4] and got[5] and not got[6]


def test_split_rule_rounds_the_threshold_to_the_dtype():
    """6.1 rounds to 6.1015625 in fp16 (and to 6.09375 in bf16): torch compares in the tensor's dtype."""
    x16 = torch.tensor([6.1015625], dtype=torch.float16)
    assert not bool(x16 > 6.1) and float(KQ.round_threshold(6.1, torch.float16)) == 6.1015625
    assert not KQ.split(x16.float().numpy(), KQ.round_threshold(6.1, torch.float16))[0][0]
    assert KQ.split(np.float32([6.1015625]), np.float32(6.1))[0][0]                   # an fp32 compare would call it an outlier
    xb = torch.tensor([6.09375, 6.125], dtype=torch.bfloat16)
    assert float(KQ.round_threshold(6.1, torch.bfloat16)) == 6.09375
    assert np.array_equal(KQ.split(xb.float().numpy(), KQ.round_threshold(6.1, torch.bfloat16))[0], _torch_mask(xb, 6.1))
    assert _kvc.outlier_threshold(6.1, torch.float16) == 6.1015625 and _kvc.outlier_threshold(6.1, torch.bfloat16) == 6.09375


# ---- the restatement against the reference's semantics ----------------------------------------------------------------------
def _data(g, b, h, rows, D, dtype):
    x = torch.randn(b, h, rows, D, generator=g) * 2
    x[:, :, :, 5] *= 20                                          # a key-like outlier channel
    x[0, 0, 3, :] = 50.0                                         # a row of outliers only
    x[:, :, 7, 9] = float("inf")
    return x.to(dtype)


@pytest.mark.parametrize("mode", [KQ.KEYS, KQ.VALUES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_restatement_matches_mask_quantize_restore(mode, dtype):
    """The reference's three steps in torch: outliers = (x < -T) | (x > T); quantize x.masked_fill(outliers, 0); de-quantize and
    write the outliers back."""
    g = torch.Generator().manual_seed(3)
    x = _data(g, 2, 3, 70, 64, dtype)
    T, nbits, G = 6.0, 2, 32
    out = torch.isfinite(x) & ~((x < -T) | (x > T))
    mask = (x < -T) | (x > T)
    dense = x.masked_fill(mask, 0)
    ref = torch.from_numpy(Q.roundtrip(dense, mode, nbits, G))
    ref[mask] = x[mask].float()
    got = KQ.roundtrip(x, mode, nbits, G, KQ.round_threshold(T, dtype))
    assert np.array_equal(got.view(np.int32), ref.numpy().view(np.int32))
    assert out.any() and mask.any()


def test_pool_layout_order_overflow_and_determinism():
    g = torch.Generator().manual_seed(4)
    x = _data(g, 2, 2, 9, 64, torch.bfloat16).float().numpy()
    mask, _ = KQ.split(x, np.float32(6.0))
    counts = mask.sum(-1)
    w, used, ri = KQ.pool_layout(x, mask, [5, 0], 10 ** 6)
    w2, used2, ri2 = KQ.pool_layout(x, mask, [5, 0], 10 ** 6)
    assert w == w2 and np.array_equal(used, used2) and np.array_equal(ri, ri2)
    for bi, base in ((0, 5), (1, 0)):
        assert used[bi] == base + counts[bi].sum()
        pos = base
        for h in range(2):
            for r in range(9):
                n = counts[bi, h, r]
                assert ri[bi, h, r] == ((pos << 8) | n if n else 0)
                pos += n
        assert [p for p, _, _ in w[bi]] == list(range(base, used[bi]))             # dense, (h, row, channel) order
    assert counts[0, 0, 4] > 0
    cap = int(counts[0, 0, :5].sum()) - 1                                          # overflow: rows that do not fit wholly are dropped
    w, used, ri = KQ.pool_layout(x, mask, [0, 0], cap)
    assert used[0] == counts[0].sum() and max(p for p, _, _ in w[0]) < cap
    assert (ri[0, 0, 4:] == 0).all() and (ri[0, 1] == 0).all()


# ---- C-ABI validation -----------------------------------------------------------------------------------------------------
def _qp(kvc, **kw):
    p = kvc.QuantParams()
    base = dict(dtype=kvc.BF16, bsz=1, n_heads=8, head_dim=128, nbits=4, group_size=64, mode=kvc.QUANT_KEYS, row0=0, rows=100,
                capacity=128, src_stride_b=8 * 100 * 128, src_stride_h=100 * 128, src_stride_l=128,
                code_stride_b=8 * 128 * 64, code_stride_h=128 * 64, meta_stride_b=8 * 2 * 2 * 128, meta_stride_h=2 * 2 * 128)
    base.update(kw)
    for k, v in base.items():
        setattr(p, k, v)
    return p


def _ol(kvc, heads=8, cap_rows=128, **kw):
    o = kvc.QuantOutliers()
    base = dict(pool_capacity=4096, pool_stride_b=4096, rowinfo_stride_h=cap_rows, rowinfo_stride_b=heads * cap_rows)
    base.update(kw)
    for k, v in base.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("kw,okw,thr,code,msg", [
    (dict(nbits=3), {}, 6.0, -1, "nbits"), (dict(head_dim=96), {}, 6.0, -2, "head_dim"), (dict(rows=129), {}, 6.0, -1, "fit"),
    ({}, {}, 0.0, -1, "threshold"), ({}, {}, -1.0, -1, "threshold"), ({}, {}, float("inf"), -1, "threshold"),
    ({}, {}, float("nan"), -1, "threshold"),
    ({}, dict(pool_capacity=-1), 6.0, -1, "pool_capacity"), ({}, dict(pool_capacity=1 << 24, pool_stride_b=1 << 24), 6.0, -1, "pool_capacity"),
    ({}, dict(pool_stride_b=100), 6.0, -1, "pool_stride_b"), ({}, dict(rowinfo_stride_h=127), 6.0, -1, "rowinfo strides"),
    ({}, dict(rowinfo_stride_b=128), 6.0, -1, "rowinfo strides"),
])
def test_quantize_outliers_rejects_invalid_arguments(kvc, kw, okw, thr, code, msg):
    L = kvc.lib()
    p, o = _qp(kvc, **kw), _ol(kvc, **okw)
    rc = L.kvc_quantize_rows_outliers(ctypes.byref(p), thr, None, None, None, ctypes.byref(o), None)
    assert rc == code, (kw, okw, rc, L.kvc_last_error())
    assert msg in L.kvc_last_error().decode()
    if thr == 6.0:
        rc = L.kvc_dequantize_rows_outliers(ctypes.byref(p), None, None, ctypes.byref(o), None, None)
        assert rc == code and msg in L.kvc_last_error().decode()


def test_quantize_outliers_valid_arguments_reach_the_pointer_checks(kvc):
    L = kvc.lib()
    p, o = _qp(kvc), _ol(kvc)
    assert L.kvc_quantize_rows_outliers(ctypes.byref(p), 6.0, None, None, None, None, None) == -1
    assert "outlier descriptor is NULL" in L.kvc_last_error().decode()
    assert L.kvc_quantize_rows_outliers(ctypes.byref(p), 6.0, None, None, None, ctypes.byref(o), None) == -1
    assert "non-NULL" in L.kvc_last_error().decode()
    assert L.kvc_dequantize_rows_outliers(ctypes.byref(p), None, None, ctypes.byref(o), None, None) == -1
    assert "non-NULL" in L.kvc_last_error().decode()
    buf = (ctypes.c_uint8 * 64)()                                    # host memory: never touched, the pool pointers are checked first
    a = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16) % 16
    rc = L.kvc_quantize_rows_outliers(ctypes.byref(p), 6.0, ctypes.c_void_p(a), ctypes.c_void_p(a), ctypes.c_void_p(a), ctypes.byref(o), None)
    assert rc == -1 and "used, rowinfo" in L.kvc_last_error().decode()
    assert L.kvc_quantize_rows_outliers(ctypes.byref(_qp(kvc, rows=0)), 6.0, None, None, None, ctypes.byref(o), None) == 0
    assert L.kvc_quantize_rows_outliers(None, 6.0, None, None, None, ctypes.byref(o), None) == -1


def _seg(kvc, rows, cap, heads, D=128, nbits=4, G=64):
    s = kvc.QuantSeg()
    s.rows, s.capacity = rows, cap
    s.code_stride_h = cap * D * nbits // 8
    s.code_stride_b = heads * s.code_stride_h
    s.k_meta_stride_h = -(-cap // G) * 2 * D
    s.k_meta_stride_b = heads * s.k_meta_stride_h
    s.v_meta_stride_h = cap * (D // G) * 2
    s.v_meta_stride_b = heads * s.v_meta_stride_h
    return s


def _dp(kvc, **kw):
    p = kvc.DecodeQuantParams()
    base = dict(dtype=kvc.BF16, bsz=1, n_q_heads=32, n_kv_heads=8, head_dim=128, nbits=4, group_size=64, residual_length=128,
                res_rows=10, res_capacity=192, new_rows=1, scaling=128 ** -0.5, q_stride_b=4096, q_stride_h=128, q_stride_l=4096,
                new_stride_b=1024, new_stride_h=128, new_stride_l=1024, res_stride_b=8 * 192 * 128, res_stride_h=192 * 128,
                out_stride_b=4096, out_stride_h=128, out_stride_l=4096)
    base.update(kw)
    for k, v in base.items():
        setattr(p, k, v)
    return p


def _pair(kvc, heads, cap_rows, **kw):
    return (kvc.QuantOutliers * 2)(_ol(kvc, heads, cap_rows, **kw), _ol(kvc, heads, cap_rows, **kw))


@pytest.mark.parametrize("kw,which,okw,code,msg", [
    (dict(nbits=5), None, {}, -1, "nbits"), (dict(res_rows=128), None, {}, -1, "res_rows"),
    ({}, "prefix", None, -1, "prefix outlier descriptors are NULL"), ({}, "tail", None, -1, "tail outlier descriptors are NULL"),
    ({}, "prefix", dict(rowinfo_stride_h=100), -1, "rowinfo strides"), ({}, "tail", dict(rowinfo_stride_b=10), -1, "rowinfo strides"),
    ({}, "prefix", dict(pool_capacity=-5), -1, "pool_capacity"), ({}, "tail", dict(pool_stride_b=1), -1, "pool_stride_b"),
])
def test_decode_step_outliers_rejects_invalid_arguments(kvc, kw, which, okw, code, msg):
    L = kvc.lib()
    p = _dp(kvc, **kw)
    pre, tail = _seg(kvc, 136, 136, 32), _seg(kvc, 128, 256, 8)
    po, to = _pair(kvc, 32, 136), _pair(kvc, 8, 256)
    if which == "prefix":
        po = None if okw is None else _pair(kvc, 32, 136, **okw)
    elif which == "tail":
        to = None if okw is None else _pair(kvc, 8, 256, **okw)
    args = (ctypes.byref(p), ctypes.byref(pre), ctypes.byref(tail), po, to)
    rc = L.kvc_decode_step_quant_outliers(*args, *([None] * 7), 0, None)
    assert rc == code, (kw, which, okw, rc, L.kvc_last_error())
    assert msg in L.kvc_last_error().decode()
    assert L.kvc_decode_quant_outliers_workspace_bytes(*args) == 0


def test_decode_step_outliers_valid_arguments(kvc):
    L = kvc.lib()
    p, pre, tail = _dp(kvc), _seg(kvc, 2056, 2056, 32), _seg(kvc, 1024, 1024, 8)
    args = (ctypes.byref(p), ctypes.byref(pre), ctypes.byref(tail), _pair(kvc, 32, 2056), _pair(kvc, 8, 1024))
    n = L.kvc_decode_quant_outliers_workspace_bytes(*args)
    assert n > 0 and n == L.kvc_decode_quant_workspace_bytes(ctypes.byref(p), ctypes.byref(pre), ctypes.byref(tail))
    rc = L.kvc_decode_step_quant_outliers(*args, *([None] * 7), 0, None)
    assert rc == -1 and "used, rowinfo" in L.kvc_last_error().decode()
    empty = _seg(kvc, 0, 0, 8)                                       # a segment without rows needs no descriptors
    assert L.kvc_decode_quant_outliers_workspace_bytes(ctypes.byref(p), ctypes.byref(pre), ctypes.byref(empty), args[3], None) > 0


def test_exports_match_the_header(kvc):
    header = open(os.path.join(ROOT, "include", "kvc.h")).read()
    new = ("kvc_quantize_rows_outliers", "kvc_dequantize_rows_outliers", "kvc_decode_quant_outliers_workspace_bytes",
           "kvc_decode_step_quant_outliers")
    for name in new:
        assert re.search(r"\b%s\(" % name, header) and name in kvc.EXPORTS
        getattr(kvc.lib(), name)
    assert "typedef struct kvc_quant_outliers" in header
    assert kvc.lib().kvc_version() == 5
    assert ctypes.sizeof(kvc.QuantOutliers) == 4 * 8 + 2 * 4 + 3 * 8


# ---- the cache object --------------------------------------------------------------------------------------------------------
def _config(layers=2):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=256, intermediate_size=128, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2,
                       head_dim=64, vocab_size=128, max_position_embeddings=2048, attn_implementation="sdpa")


def test_cache_arguments():
    import kvcache_factory_amd as pkg
    from kvcache_factory_amd import KVQuantCompressedCache, KVQuantCompressedLayer, QuantizedCompressedCache
    assert "KVQuantCompressedCache" in pkg.__all__ and "KVQuantCompressedLayer" in pkg.__all__
    c = KVQuantCompressedCache(_config(3), nbits=2, q_group_size=32, residual_length=64, outlier_threshold=4.5)
    assert isinstance(c, QuantizedCompressedCache) and len(c.layers) == 3
    assert all(isinstance(x, KVQuantCompressedLayer) for x in c.layers)
    assert (c.layers[0].nbits, c.layers[0].group_size, c.layers[0].residual_length, c.layers[0].outlier_threshold) == (2, 32, 64, 4.5)
    d = KVQuantCompressedCache(_config())
    assert (d.nbits, d.q_group_size, d.residual_length, d.outlier_threshold) == (4, 64, 128, 6.0)
    for kw in (dict(outlier_threshold=0), dict(outlier_threshold=-1.0), dict(outlier_threshold=float("inf")),
               dict(outlier_threshold=float("nan")), dict(nbits=3), dict(q_group_size=64, residual_length=96)):
        with pytest.raises(ValueError):
            KVQuantCompressedCache(_config(), **kw)
    with pytest.raises(ValueError, match="not configurable"):
        KVQuantCompressedCache(_config(), backend="hqq")
    with pytest.raises(ValueError):
        KVQuantCompressedLayer(outlier_threshold=0.0)


@pytest.mark.parametrize("method", ["adakv", "headkv", "think"])
def test_adakv_headkv_think_refuse_the_kvquant_cache(method):
    from transformers import LlamaForCausalLM
    from kvcache_factory_amd import KVQuantCompressedCache, monkeypatch as mp
    torch.manual_seed(0)
    model = LlamaForCausalLM(_config()).eval()
    cache = KVQuantCompressedCache(model.config)
    layers = list(cache.layers)
    try:
        mp.replace_llama(method)
        with pytest.raises(NotImplementedError, match="QuantizedCompressedCache"):
            with torch.no_grad():
                model(torch.randint(0, 128, (1, 40)), past_key_values=cache, use_cache=True)
    finally:
        mp.replace_llama("fullkv")
    assert all(a is b for a, b in zip(cache.layers, layers))


# ---- layer bookkeeping on the CPU --------------------------------------------------------------------------------------------
@pytest.fixture()
def kvq_cpu(monkeypatch):
    monkeypatch.setattr(_kvc, "quantize_rows", Q.quantize_rows)
    monkeypatch.setattr(_kvc, "dequantize_rows", Q.dequantize_rows)
    monkeypatch.setattr(_kvc, "decode_step_quant", Q.decode_step_quant)
    monkeypatch.setattr(_kvc, "quantize_rows_outliers", KQ.quantize_rows_outliers)
    monkeypatch.setattr(_kvc, "dequantize_rows_outliers", KQ.dequantize_rows_outliers)
    monkeypatch.setattr(_kvc, "decode_step_quant_outliers", KQ.decode_step_quant_outliers)

    def outlier_pool(bsz, n_heads, capacity, pool_capacity, dtype, device):        # zeroed: byte comparisons of whole pools
        return (torch.zeros(bsz, pool_capacity, dtype=torch.uint8), torch.zeros(bsz, pool_capacity, dtype=dtype),
                torch.zeros(bsz, dtype=torch.int32), torch.zeros(bsz, n_heads, capacity, dtype=torch.int32))
    monkeypatch.setattr(_kvc, "outlier_pool", outlier_pool)
    yield


def _bf(g, *sh, spike=0.0):
    x = torch.randn(*sh, generator=g)
    if spike:
        x[..., 3] *= spike                                           # an outlier channel
    return x.to(torch.bfloat16)


def _count_reads(layer, monkeypatch):
    calls = []
    orig = layer._read_used
    monkeypatch.setattr(layer, "_read_used", lambda *p: calls.append(len(p)) or orig(*p))
    return calls


@pytest.mark.parametrize("form", ["fused", "shaped"])
def test_layer_flush_pool_growth_and_host_reads(kvq_cpu, monkeypatch, form):
    """G = R = 32, D = 64, two KV heads: residual flush as in the KIVI layer; pool entries, used and rowinfo words stay byte for byte
    across later flushes; `used` is read back once at the first decode step and never by a step that does not grow the pool; the layer's keys / values are the restated de-quantized cache with the outliers exact."""
    from kvcache_factory_amd.cache import KVQuantCompressedLayer
    g = torch.Generator().manual_seed(21)
    hq, hkv, D, P, G = 4, 2, 64, 45, 32
    k0, v0 = _bf(g, 1, hq, P, D, spike=8), _bf(g, 1, hq, P, D, spike=8)
    layer = KVQuantCompressedLayer(nbits=2, q_group_size=G, residual_length=G, outlier_threshold=3.0)
    reads = _count_reads(layer, monkeypatch)
    layer.prefill(k0, v0, 1000)
    heads = hkv if form == "fused" else hq
    W = G * D * heads
    rows_k, rows_v, snap, flushes, reads_at = [], [], None, 0, []
    for step in range(7 * G + 1):
        kn, vn = _bf(g, 1, heads, 1, D, spike=8), _bf(g, 1, heads, 1, D, spike=8)
        before = len(reads)
        trows = layer._trows
        if form == "fused":
            layer.decode_attend(_bf(g, 1, hq, 1, D), kn, vn, D ** -0.5)
        else:
            layer.update(kn, vn)
        rows_k.append(kn)
        rows_v.append(vn)
        if step == 0:
            assert len(reads) == 1 and reads[0] == 2                  # the prompt: one read of both pools
            pk = layer._pool("_pko")
            assert pk[0].shape[1] == max(16, -(-int(pk[2].max()) // 16) * 16)
        elif layer._trows == trows:
            assert len(reads) == before                               # a step without a flush reads nothing
        else:
            flushes += 1
            if len(reads) > before:
                reads_at.append(flushes)
        if layer._trows:
            tk = layer._pool("_tko")
            used = int(tk[2].max())
            assert used <= tk[0].shape[1] and layer._tbound >= used
            if snap is not None:
                for a, b in zip(snap, (tk[0], tk[1], tk[3])):
                    n = a.shape[1] if a.dim() == 2 else a.shape[2]
                    assert torch.equal(a, b[:, :n] if a.dim() == 2 else b[:, :, :n])
            snap = (tk[0][:, :used].clone(), tk[1][:, :used].clone(), tk[3][:, :, :layer._trows].clone())
    assert flushes == 7 and reads_at == []                            # the bound follows the copies of used: no read, no growth
    assert layer._pool("_tko")[0].shape[1] == 2 * W
    # keys / values: the restated cache
    rep = hq // heads
    allk, allv = torch.cat(rows_k, 2), torch.cat(rows_v, 2)
    q = layer._trows
    thr = KQ.round_threshold(3.0, torch.bfloat16)
    exp_k = np.concatenate([KQ.roundtrip(k0, Q.KEYS, 2, G, thr),
                            np.concatenate([KQ.roundtrip(allk[:, :, i:i + G], Q.KEYS, 2, G, thr) for i in range(0, q, G)], 2).repeat(rep, 1),
                            allk[:, :, q:].float().numpy().repeat(rep, 1)], 2)
    exp_v = np.concatenate([KQ.roundtrip(v0, Q.VALUES, 2, G, thr), KQ.roundtrip(allv[:, :, :q], Q.VALUES, 2, G, thr).repeat(rep, 1),
                            allv[:, :, q:].float().numpy().repeat(rep, 1)], 2)
    assert np.array_equal(layer.keys.float().numpy(), torch.from_numpy(exp_k).to(torch.bfloat16).float().numpy())
    assert np.array_equal(layer.values.float().numpy(), torch.from_numpy(exp_v).to(torch.bfloat16).float().numpy())


def test_tail_pool_grows_byte_for_byte(kvq_cpu, monkeypatch):
    """A pool that would fall below one worst-case flush of headroom grows; its entries are copied byte for byte."""
    from kvcache_factory_amd.cache import KVQuantCompressedLayer
    g = torch.Generator().manual_seed(22)
    layer = KVQuantCompressedLayer(nbits=4, q_group_size=32, residual_length=32, outlier_threshold=0.5)   # most elements are outliers
    reads = _count_reads(layer, monkeypatch)
    layer.prefill(_bf(g, 1, 4, 40, 64), _bf(g, 1, 4, 40, 64), 300)
    caps, snaps = [], []
    for _ in range(6 * 32):
        layer.decode_attend(_bf(g, 1, 4, 1, 64), _bf(g, 1, 2, 1, 64), _bf(g, 1, 2, 1, 64), 0.125)
        tk = layer._pool("_tko")
        if tk is not None:
            if caps and tk[0].shape[1] != caps[-1]:
                c, v = snaps[-1]
                assert torch.equal(tk[0][:, :c.shape[1]], c) and torch.equal(tk[1][:, :v.shape[1]].view(torch.int16), v.view(torch.int16))
            caps.append(tk[0].shape[1])
            u = int(tk[2].max())
            assert u <= caps[-1]
            snaps.append((tk[0][:, :u].clone(), tk[1][:, :u].clone()))
    assert len(set(caps)) >= 2 and caps == sorted(caps)
    assert len(reads) - 1 == len(set(caps)) - 1                       # after the prompt's read: one read per growth
    kk = layer.keys
    assert kk.shape == (1, 4, 40 + 6 * 32, 64)


def test_beam_reordering_permutes_the_pools(kvq_cpu):
    from kvcache_factory_amd.cache import KVQuantCompressedLayer
    g = torch.Generator().manual_seed(8)
    layer = KVQuantCompressedLayer(nbits=4, q_group_size=32, residual_length=32, outlier_threshold=2.0)
    layer.prefill(_bf(g, 3, 4, 40, 64, spike=5), _bf(g, 3, 4, 40, 64, spike=5), 300)
    for _ in range(35):
        layer.update(_bf(g, 3, 4, 1, 64, spike=5), _bf(g, 3, 4, 1, 64, spike=5))
    names = [n for n in layer._batch_tensors if getattr(layer, n) is not None]
    pools = {f"{p}_{x}" for p in ("_pko", "_pvo", "_tko", "_tvo") for x in ("chan", "val", "used", "ri")}
    assert pools <= set(names)
    before = {n: getattr(layer, n).clone() for n in names}
    kk, vv = layer.keys, layer.values
    beam = torch.tensor([2, 0, 0])
    layer.reorder_cache(beam)
    for n in names:
        assert torch.equal(getattr(layer, n).contiguous().view(torch.uint8), before[n][beam].contiguous().view(torch.uint8)), n
    assert torch.equal(layer.keys, kk[beam]) and torch.equal(layer.values, vv[beam])


def test_fullkv_generates_with_the_kvquant_cache_on_cpu(kvq_cpu, monkeypatch):
    from transformers import LlamaForCausalLM
    from kvcache_factory_amd import KVQuantCompressedCache
    torch.manual_seed(0)
    model = LlamaForCausalLM(_config()).eval()
    cache = KVQuantCompressedCache(model.config, nbits=8, q_group_size=32, residual_length=32, outlier_threshold=1.0)
    reads = [_count_reads(layer, monkeypatch) for layer in cache.layers]
    ids = torch.randint(0, 128, (1, 50), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        out = model.generate(ids, max_new_tokens=40, do_sample=False, past_key_values=cache, return_dict_in_generate=True)
    assert out.sequences.shape == (1, 90)
    layer = out.past_key_values.layers[0]
    assert layer.get_seq_length() == 89 and layer._trows == 32 and layer._rrows == 7
    assert int(layer._pool("_pko")[2].max()) > 0 and int(layer._pool("_tko")[2].max()) > 0
    assert [len(r) for r in reads] == [1, 1]                           # the prompt's read; one flush fits the tail pool's bound
