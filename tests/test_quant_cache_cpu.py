"""The quantized decode cache without a GPU: the C-ABI rejects every invalid argument before touching a pointer,
QuantizedCompressedCache checks its arguments, AdaKV / HeadKV / ThinK refuse it, and the layer's bookkeeping (residual flush,
lengths, mask sizes, append-only quantized tail, both decode forms, beam reordering) holds with the `_kvc` quant entry points
replaced by the numpy restatement of tests/quant_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

import quant_ref as Q
from kvcache_factory_amd import _kvc


# ---- C-ABI validation (null pointers: nothing may be touched before the arguments are checked) --------------------------------
def _qp(kvc, **kw):
    p = kvc.QuantParams()
    base = dict(dtype=kvc.BF16, bsz=1, n_heads=8, head_dim=128, nbits=4, group_size=64, mode=kvc.QUANT_KEYS, row0=0, rows=100,
                capacity=128, src_stride_b=8 * 100 * 128, src_stride_h=100 * 128, src_stride_l=128,
                code_stride_b=8 * 128 * 64, code_stride_h=128 * 64, meta_stride_b=8 * 2 * 2 * 128, meta_stride_h=2 * 2 * 128)
    base.update(kw)
    for k, v in base.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw,code,msg", [
    (dict(nbits=3), -1, "nbits"), (dict(nbits=16), -1, "nbits"), (dict(nbits=1), -1, "nbits"),
    (dict(group_size=128, head_dim=64), -1, "divide"),
    (dict(group_size=48), -2, "group_size"),
    (dict(dtype=7), -1, "dtype"),
    (dict(head_dim=96), -2, "head_dim"),
    (dict(mode=2), -1, "mode"),
    (dict(rows=129), -1, "fit"), (dict(row0=64, rows=100), -1, "fit"),
    (dict(row0=32, rows=10), -1, "group boundary"),
    (dict(code_stride_h=128 * 64 - 16), -1, "code strides"),
    (dict(meta_stride_h=2 * 128), -1, "metadata strides"),
    (dict(mode=1, meta_stride_h=128 * 2 * 2 - 4, meta_stride_b=8 * 128 * 4), -1, "metadata strides"),
    (dict(src_stride_l=64), -1, "strides"),
])
def test_quantize_rejects_invalid_arguments(kvc, kw, code, msg):
    L = kvc.lib()
    p = _qp(kvc, **kw)
    for fn in (L.kvc_quantize_rows, L.kvc_dequantize_rows):
        rc = fn(ctypes.byref(p), None, None, None, None)
        assert rc == code, (kw, rc, L.kvc_last_error())
        assert msg in L.kvc_last_error().decode()


def test_quantize_valid_arguments_reach_the_pointer_checks(kvc):
    L = kvc.lib()
    assert L.kvc_quantize_rows(ctypes.byref(_qp(kvc)), None, None, None, None) == -1
    assert "non-NULL" in L.kvc_last_error().decode()
    assert L.kvc_quantize_rows(ctypes.byref(_qp(kvc, rows=0)), None, None, None, None) == 0      # nothing to do
    assert L.kvc_quantize_rows(None, None, None, None, None) == -1


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


@pytest.mark.parametrize("kw,seg,code,msg", [
    (dict(nbits=5), None, -1, "nbits"),
    (dict(group_size=128, head_dim=64), None, -1, "divide"),
    (dict(residual_length=96), None, -1, "multiple of group_size"),
    (dict(residual_length=0), None, -1, "multiple of group_size"),
    (dict(dtype=3), None, -1, "dtype"),
    (dict(head_dim=256), None, -2, "head_dim"),
    (dict(res_rows=128), None, -1, "res_rows"),
    (dict(new_rows=0), None, -1, "new_rows"),
    (dict(res_rows=100, new_rows=100), None, -1, "fit"),
    (dict(res_stride_h=100 * 128), None, -1, "residual strides"),
    (dict(n_kv_heads=5), None, -1, "head counts"),
    ({}, ("prefix", dict(rows=300)), -1, "fit"),
    ({}, ("prefix", dict(code_stride_h=64)), -1, "strides"),
    ({}, ("tail", dict(rows=100)), -1, "multiple of group_size"),
    ({}, ("tail", dict(k_meta_stride_h=4)), -1, "strides"),
])
def test_decode_step_quant_rejects_invalid_arguments(kvc, kw, seg, code, msg):
    L = kvc.lib()
    p = _dp(kvc, **kw)
    pre, tail = _seg(kvc, 136, 136, 32), _seg(kvc, 128, 256, 8)
    if seg:
        tgt = pre if seg[0] == "prefix" else tail
        for k, v in seg[1].items():
            setattr(tgt, k, v)
    rc = L.kvc_decode_step_quant(ctypes.byref(p), ctypes.byref(pre), ctypes.byref(tail), *([None] * 7), 0, None)
    assert rc == code, (kw, seg, rc, L.kvc_last_error())
    assert msg in L.kvc_last_error().decode()
    assert L.kvc_decode_quant_workspace_bytes(ctypes.byref(p), ctypes.byref(pre), ctypes.byref(tail)) == 0
    assert L.kvc_decode_step_quant(ctypes.byref(_dp(kvc)), None, ctypes.byref(tail), *([None] * 7), 0, None) == -1


def test_decode_step_quant_valid_arguments(kvc):
    L = kvc.lib()
    p, pre, tail = _dp(kvc), _seg(kvc, 2056, 2056, 32), _seg(kvc, 1024, 1024, 8)
    assert L.kvc_decode_quant_workspace_bytes(ctypes.byref(p), ctypes.byref(pre), ctypes.byref(tail)) > 0
    rc = L.kvc_decode_step_quant(ctypes.byref(p), ctypes.byref(pre), ctypes.byref(tail), *([None] * 7), 0, None)
    assert rc == -1 and "non-NULL" in L.kvc_last_error().decode()


# ---- the cache object --------------------------------------------------------------------------------------------------------
def _config(layers=2):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=256, intermediate_size=128, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2,
                       head_dim=64, vocab_size=128, max_position_embeddings=2048, attn_implementation="sdpa")


def test_cache_arguments():
    from kvcache_factory_amd import QuantizedCompressedCache, QuantizedCompressedLayer
    c = QuantizedCompressedCache(_config(3), nbits=2, q_group_size=32, residual_length=64)
    assert len(c.layers) == 3 and all(isinstance(x, QuantizedCompressedLayer) for x in c.layers)
    assert (c.layers[0].nbits, c.layers[0].group_size, c.layers[0].residual_length) == (2, 32, 64)
    d = QuantizedCompressedCache(_config())
    assert (d.nbits, d.q_group_size, d.residual_length) == (4, 64, 128)
    for kw in (dict(backend="quanto"), dict(backend="hqq"), dict(axis_key=0), dict(axis_value=1)):
        with pytest.raises(ValueError, match="not configurable"):
            QuantizedCompressedCache(_config(), **kw)
    for kw in (dict(nbits=3), dict(nbits=16), dict(q_group_size=16), dict(q_group_size=64, residual_length=96),
               dict(q_group_size=32, residual_length=0)):
        with pytest.raises(ValueError):
            QuantizedCompressedCache(_config(), **kw)


@pytest.mark.parametrize("method", ["adakv", "headkv", "think"])
def test_adakv_headkv_think_refuse_the_quantized_cache(method):
    from transformers import LlamaForCausalLM
    from kvcache_factory_amd import QuantizedCompressedCache, monkeypatch as mp
    torch.manual_seed(0)
    model = LlamaForCausalLM(_config()).eval()
    cache = QuantizedCompressedCache(model.config)
    layers = list(cache.layers)
    try:
        mp.replace_llama(method)
        with pytest.raises(NotImplementedError, match="QuantizedCompressedCache"):
            with torch.no_grad():
                model(torch.randint(0, 128, (1, 40)), past_key_values=cache, use_cache=True)
    finally:
        mp.replace_llama("fullkv")
    assert all(a is b for a, b in zip(cache.layers, layers))                # nothing replaced


# ---- layer bookkeeping on the CPU --------------------------------------------------------------------------------------------
@pytest.fixture()
def quant_cpu(monkeypatch):
    monkeypatch.setattr(_kvc, "quantize_rows", Q.quantize_rows)
    monkeypatch.setattr(_kvc, "dequantize_rows", Q.dequantize_rows)
    monkeypatch.setattr(_kvc, "decode_step_quant", Q.decode_step_quant)
    yield


def _bf(g, *sh):
    return torch.randn(*sh, generator=g).to(torch.bfloat16)


def _segment_codes(layer):
    return [x[:, :, :n].clone() for x, n in ((layer._tkc, layer._trows), (layer._tvc, layer._trows),
                                             (layer._tkm, layer._trows // layer.group_size), (layer._tvm, layer._trows))]


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("form", ["fused", "shaped"])
def test_layer_residual_flush(quant_cpu, t, form):
    """Residual flush at R (G = R = 32): after every step the residual holds < R rows, floor(rows / G) * G rows went to the
    quantized tail; lengths and mask sizes; quantized blocks stay byte for byte across later flushes (and a capacity growth);
    the layer's `keys` / `values` are the de-quantized prefix + blocks + the full-precision residual."""
    from kvcache_factory_amd.cache import QuantizedCompressedLayer
    g = torch.Generator().manual_seed(11 + t)
    hq, hkv, D, P, G = 4, 2, 64, 45, 32
    k0, v0 = _bf(g, 1, hq, P, D), _bf(g, 1, hq, P, D)
    layer = QuantizedCompressedLayer(nbits=4, q_group_size=G, residual_length=G)
    layer.prefill(k0, v0, 1000)
    assert layer.keys.shape == (1, hq, P, D) and layer._kbuf is not None
    rows_k, rows_v, snap, res = [], [], None, 0
    heads = hkv if form == "fused" else hq
    for step in range(5 * G // t + 3):                                   # past 4 * R quantized rows: the tail grows once
        kn, vn = _bf(g, 1, heads, t, D), _bf(g, 1, heads, t, D)
        if form == "fused":
            out = layer.decode_attend(_bf(g, 1, hq, t, D), kn, vn, D ** -0.5)
            assert out.shape == (1, t, hq, D)
        else:
            k, v = layer.update(kn, vn)
            assert k.shape == (1, hq, P + (len(rows_k) + 1) * t, D)
        assert layer._kbuf is None and layer._vbuf is None and layer._prows == P      # the prompt buffers are gone
        rows_k.append(kn)
        rows_v.append(vn)
        res += t
        if res >= G:
            res -= res // G * G
        n = len(rows_k) * t
        assert layer._rrows == res and layer._trows == n - res and layer._trows % G == 0
        assert layer.get_seq_length() == 1000 + n
        assert layer.stored_length() == P + n and layer.get_mask_sizes(1) == (P + n + 1, 0)
        if snap is not None:
            for a, b in zip(snap, _segment_codes(layer)):
                assert torch.equal(a, b[:, :, :a.shape[2]])
        if layer._trows:
            snap = _segment_codes(layer)
    assert layer._tkc.shape[2] > 4 * G                                   # grew at least once
    allk, allv = torch.cat(rows_k, 2), torch.cat(rows_v, 2)
    q = layer._trows
    rep = hq // heads
    exp_k = np.concatenate([Q.roundtrip(k0, Q.KEYS, 4, G),
                            np.concatenate([Q.roundtrip(allk[:, :, i:i + G], Q.KEYS, 4, G) for i in range(0, q, G)], 2).repeat(rep, 1),
                            allk[:, :, q:].float().numpy().repeat(rep, 1)], 2)
    exp_v = np.concatenate([Q.roundtrip(v0, Q.VALUES, 4, G), Q.roundtrip(allv[:, :, :q], Q.VALUES, 4, G).repeat(rep, 1),
                            allv[:, :, q:].float().numpy().repeat(rep, 1)], 2)
    assert np.array_equal(layer.keys.float().numpy(), torch.from_numpy(exp_k).to(torch.bfloat16).float().numpy())
    assert np.array_equal(layer.values.float().numpy(), torch.from_numpy(exp_v).to(torch.bfloat16).float().numpy())


def test_layer_refuses_to_switch_forms(quant_cpu):
    from kvcache_factory_amd.cache import QuantizedCompressedLayer
    g = torch.Generator().manual_seed(5)
    for first in ("fused", "shaped"):
        layer = QuantizedCompressedLayer(nbits=2, q_group_size=32, residual_length=64)
        layer.prefill(_bf(g, 1, 4, 40, 64), _bf(g, 1, 4, 40, 64), 500)
        fused = lambda: layer.decode_attend(_bf(g, 1, 4, 1, 64), _bf(g, 1, 2, 1, 64), _bf(g, 1, 2, 1, 64), 0.125)   # noqa: E731
        shaped = lambda: layer.update(_bf(g, 1, 4, 1, 64), _bf(g, 1, 4, 1, 64))                                    # noqa: E731
        a, b = (fused, shaped) if first == "fused" else (shaped, fused)
        a()
        with pytest.raises(RuntimeError, match="switch"):
            b()
        layer.reset()
        assert layer.get_seq_length() == 0 and layer.keys is None and layer._mode is None and layer.stored_length() == 0


def test_layer_without_prefill_takes_the_prefix_from_update(quant_cpu):
    """fullkv: the first update is the prompt — returned unquantized, as transformers' quantized cache does."""
    from kvcache_factory_amd.cache import QuantizedCompressedLayer
    g = torch.Generator().manual_seed(6)
    layer = QuantizedCompressedLayer(nbits=8, q_group_size=32, residual_length=32)
    k0, v0 = _bf(g, 1, 2, 70, 64), _bf(g, 1, 2, 70, 64)
    k, v = layer.update(k0, v0)
    assert k is k0 and v is v0 and layer.get_seq_length() == 70 and layer._prows == 70
    k, v = layer.update(_bf(g, 1, 2, 1, 64), _bf(g, 1, 2, 1, 64))
    assert k.shape == (1, 2, 71, 64) and layer.get_mask_sizes(1) == (72, 0)
    assert np.array_equal(k[:, :, :70].float().numpy(), torch.from_numpy(Q.roundtrip(k0, Q.KEYS, 8, 32)).to(torch.bfloat16).float().numpy())


def test_fullkv_generates_with_the_quantized_cache_on_cpu(quant_cpu):
    from transformers import LlamaForCausalLM
    from kvcache_factory_amd import QuantizedCompressedCache
    torch.manual_seed(0)
    model = LlamaForCausalLM(_config()).eval()
    cache = QuantizedCompressedCache(model.config, nbits=8, q_group_size=32, residual_length=32)
    ids = torch.randint(0, 128, (1, 50), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        out = model.generate(ids, max_new_tokens=40, do_sample=False, past_key_values=cache, return_dict_in_generate=True)
    assert out.sequences.shape == (1, 90)
    layer = out.past_key_values.layers[0]
    assert layer.get_seq_length() == 89 and layer._trows == 32 and layer._rrows == 7


def test_beam_reordering_permutes_every_quantized_buffer(quant_cpu):
    from kvcache_factory_amd.cache import QuantizedCompressedLayer
    g = torch.Generator().manual_seed(8)
    layer = QuantizedCompressedLayer(nbits=4, q_group_size=32, residual_length=32)
    layer.prefill(_bf(g, 3, 4, 40, 64), _bf(g, 3, 4, 40, 64), 300)
    for _ in range(35):
        layer.update(_bf(g, 3, 4, 1, 64), _bf(g, 3, 4, 1, 64))
    names = [n for n in layer._batch_tensors if getattr(layer, n) is not None]
    assert set(names) == {"_pkc", "_pvc", "_pkm", "_pvm", "_tkc", "_tvc", "_tkm", "_tvm", "_rk", "_rv"}
    before = {n: getattr(layer, n).clone() for n in names}
    kk = layer.keys
    beam = torch.tensor([2, 0, 0])
    layer.reorder_cache(beam)
    for n in names:                                                   # bytes: spare rows are uninitialised (NaN != NaN)
        assert torch.equal(getattr(layer, n).contiguous().view(torch.uint8), before[n][beam].contiguous().view(torch.uint8)), n
    assert torch.equal(layer.keys, kk[beam])
