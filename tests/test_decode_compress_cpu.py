"""Decode-stage compression without a GPU: kvc_decode_compress argument checks (every field, null pointers), the
DecodeCompressedCache arguments and refusals, and the layer's bookkeeping with the kernels replaced by CPU stand-ins
(the decode compression by the oracle on the materialised cache): trigger steps, budgets, the query ring, lengths, beams."""
import ctypes

import pytest
import torch

from cpu_compress import oracle_compress, oracle_compress_batch, oracle_decode_step
from kvcache_factory_amd import _kvc


# ---- C-ABI argument checks ---------------------------------------------------------------------------------------------------
def _dp(kvc, **kw):
    p = kvc.DecodeCompressParams()
    base = dict(method=kvc.SNAPKV, dtype=kvc.BF16, bsz=1, n_q_heads=32, n_kv_heads=8, head_dim=128, prefix_rows=2048, tail_rows=128,
                window=32, k=2016, kernel_size=7, pooling=kvc.POOL_MAX, tie_mode=kvc.TIES_TORCH_CPU, ring_start=5,
                ring_stride_b=32 * 32 * 128, ring_stride_h=32 * 128, prefix_stride_b=32 * 2304 * 128, prefix_stride_h=2304 * 128,
                tail_stride_b=8 * 256 * 128, tail_stride_h=256 * 128, out_stride_b=32 * 2048 * 128, out_stride_h=2048 * 128)
    base.update(kw)
    for k, v in base.items():
        setattr(p, k, v)
    return p


def test_params_struct_matches_header(kvc):
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kvc.h")).read()
    body = text[text.index("typedef struct kvc_decode_compress_params {"):text.index("} kvc_decode_compress_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in re.findall(r"int(?:32|64)_t\s+([^;]+);", body):
        fields += [f.strip() for f in decl.split(",")]
    assert fields == [f[0] for f in kvc.DecodeCompressParams._fields_]
    assert ctypes.sizeof(kvc.DecodeCompressParams) == 14 * 4 + 8 * 8
    assert {"kvc_decode_compress", "kvc_decode_compress_workspace_bytes"} <= set(kvc.EXPORTS)


def test_workspace_bytes(kvc):
    L = kvc.lib()
    n = L.kvc_decode_compress_workspace_bytes(ctypes.byref(_dp(kvc)))
    # at least the logits [32][2176][32] bf16 and the scores [32][2144] of the equivalent kvc_compress call
    assert n >= 32 * 2176 * 32 * 2 + 32 * 2144 * 2 and n % 256 == 0
    assert L.kvc_decode_compress_workspace_bytes(ctypes.byref(_dp(kvc, method=kvc.STREAMINGLLM))) == 0
    assert L.kvc_last_error() == b""
    assert L.kvc_decode_compress_workspace_bytes(ctypes.byref(_dp(kvc, window=65))) == 0
    assert b"window" in L.kvc_last_error()


BAD = [
    (dict(method=2), -1, "method 2"), (dict(method=4), -1, "method 4"), (dict(dtype=3), -1, "dtype"),
    (dict(bsz=0), -1, "positive"), (dict(n_q_heads=0), -1, "positive"), (dict(n_kv_heads=0), -1, "positive"),
    (dict(n_kv_heads=5), -1, "multiple"), (dict(head_dim=96), -2, "head_dim"), (dict(window=0), -1, "window"),
    (dict(window=65), -2, "window 65"), (dict(prefix_rows=-1), -1, "prefix_rows"), (dict(tail_rows=31), -1, "tail_rows 31"),
    (dict(prefix_rows=0, tail_rows=32), -1, "must exceed window"), (dict(k=-1), -1, "k=-1"), (dict(k=2145), -1, "k=2145"),
    (dict(tie_mode=2), -1, "tie_mode"), (dict(pooling=3), -1, "Pooling"), (dict(kernel_size=0), -2, "kernel_size"),
    (dict(kernel_size=65), -2, "kernel_size"), (dict(kernel_size=6), -2, "even kernel_size"), (dict(ring_start=32), -1, "ring_start"),
    (dict(ring_start=-1), -1, "ring_start"),
    (dict(tie_mode=1, prefix_rows=200000, k=16385, prefix_stride_h=200000 * 128, prefix_stride_b=32 * 200000 * 128,
          out_stride_h=16417 * 128, out_stride_b=32 * 16417 * 128), -2, "canonical"),
    (dict(prefix_rows=2000000, k=18001, prefix_stride_h=2000000 * 128, prefix_stride_b=32 * 2000000 * 128,
          out_stride_h=18033 * 128, out_stride_b=32 * 18033 * 128), -2, "partial_sort"),
    (dict(ring_stride_h=32 * 128 + 4), -4, "ring strides"), (dict(ring_stride_h=31 * 128), -1, "ring strides"),
    (dict(prefix_stride_b=3), -4, "prefix strides"), (dict(prefix_stride_h=2047 * 128), -1, "prefix strides"),
    (dict(tail_stride_h=127 * 128), -1, "tail strides"), (dict(tail_stride_b=7 * 256 * 128), -1, "tail strides"),
    (dict(out_stride_h=2047 * 128), -1, "out strides"), (dict(out_stride_b=4), -4, "out strides"),
]


@pytest.mark.parametrize("kw,code,msg", BAD, ids=[f"{list(b[0])[0]}={list(b[0].values())[0]}" for b in BAD])
def test_invalid_params_rejected_before_any_pointer(kvc, kw, code, msg):
    L = kvc.lib()
    rc = L.kvc_decode_compress(ctypes.byref(_dp(kvc, **kw)), *([None] * 10), 0, None)
    assert rc == code and msg in L.kvc_last_error().decode(), (rc, L.kvc_last_error())
    assert L.kvc_decode_compress_workspace_bytes(ctypes.byref(_dp(kvc, **kw))) == 0


def test_null_params_and_pointers(kvc):
    L = kvc.lib()
    assert L.kvc_decode_compress(None, *([None] * 10), 0, None) == -1 and b"NULL" in L.kvc_last_error()
    rc = L.kvc_decode_compress(ctypes.byref(_dp(kvc)), *([None] * 10), 0, None)
    assert rc == -1 and b"non-NULL" in L.kvc_last_error()
    a = ctypes.c_void_p(1 << 40)                                  # never dereferenced: the checks below come first
    bad = ctypes.c_void_p((1 << 40) + 8)
    p = _dp(kvc)
    rc = L.kvc_decode_compress(ctypes.byref(p), None, a, a, a, a, a, a, None, None, None, 0, None)
    assert rc == -1 and b"q_ring" in L.kvc_last_error()
    rc = L.kvc_decode_compress(ctypes.byref(p), a, None, a, a, a, a, a, None, None, None, 0, None)
    assert rc == -1 and b"k_prefix" in L.kvc_last_error()
    rc = L.kvc_decode_compress(ctypes.byref(p), a, a, a, bad, a, a, a, None, None, None, 0, None)
    assert rc == -4 and b"aligned" in L.kvc_last_error()
    rc = L.kvc_decode_compress(ctypes.byref(_dp(kvc, method=kvc.STREAMINGLLM)), None, a, a, a, a, a, a,
                               ctypes.c_void_p(1 << 41), None, None, 0, None)
    assert rc == -2 and b"idx_out must be NULL" in L.kvc_last_error()


def test_overlapping_outputs_and_workspace_rejected(kvc):
    L = kvc.lib()
    p = _dp(kvc)
    base = 1 << 40
    ptr = lambda off: ctypes.c_void_p(base + off)
    pre_b = 32 * 2304 * 128 * 2                                   # bytes of one prefix buffer
    tail_b = 8 * 256 * 128 * 2
    kp, vp, kt, vt = 0, pre_b, 2 * pre_b, 2 * pre_b + tail_b
    free = 2 * pre_b + 2 * tail_b
    out_b = 32 * 2048 * 128 * 2
    for ko, vo in ((kp, free + out_b), (free, vp + 4096), (free, kt), (free, free + out_b // 2), (vt - 4096, free + out_b)):
        rc = L.kvc_decode_compress(ctypes.byref(p), ptr(1 << 30), ptr(kp), ptr(vp), ptr(kt), ptr(vt), ptr(ko), ptr(vo), None, None,
                                   None, 0, None)
        assert rc == -1 and b"overlap" in L.kvc_last_error(), (ko, vo)
    args = (ptr(1 << 30), ptr(kp), ptr(vp), ptr(kt), ptr(vt), ptr(free), ptr(free + out_b), None, None)
    need = L.kvc_decode_compress_workspace_bytes(ctypes.byref(p))
    assert L.kvc_decode_compress(ctypes.byref(p), *args, None, 0, None) == -3
    assert L.kvc_decode_compress(ctypes.byref(p), *args, ptr(1 << 35 | 128), need, None) == -3
    assert L.kvc_decode_compress(ctypes.byref(p), *args, ptr(1 << 35), need - 256, None) == -3
    assert b"too small" in L.kvc_last_error()


# ---- the cache object --------------------------------------------------------------------------------------------------------
def _config(layers=2):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=256, intermediate_size=128, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2,
                       head_dim=64, vocab_size=128, max_position_embeddings=2048, attn_implementation="sdpa")


def test_cache_arguments():
    from kvcache_factory_amd import DecodeCompressedCache, DecodeCompressedLayer
    from kvcache_factory_amd.cache import CompressedDynamicLayer
    c = DecodeCompressedCache(_config(3), interval=64)
    assert len(c.layers) == 3 and all(isinstance(x, DecodeCompressedLayer) for x in c.layers)
    assert issubclass(DecodeCompressedLayer, CompressedDynamicLayer)
    assert c.interval == 64 and c.layers[0].interval == 64 and DecodeCompressedCache(_config()).layers[1].interval == 128
    for bad in (0, -3, 1.5, True, "8", None):
        with pytest.raises(ValueError, match="interval"):
            DecodeCompressedCache(_config(), interval=bad)
        with pytest.raises(ValueError, match="interval"):
            DecodeCompressedLayer(bad)


def _run_model(method, cache, L=40, steps=1, merge=None, cap=64, W=8):
    from transformers import LlamaForCausalLM
    from kvcache_factory_amd import monkeypatch as mp
    torch.manual_seed(0)
    model = LlamaForCausalLM(_config()).eval()
    try:
        mp.replace_llama(method)
        for layer in model.model.layers:
            for name, val in (("window_size", W), ("max_capacity_prompt", cap), ("kernel_size", 7), ("pooling", "maxpool"),
                              ("merge", merge)):
                setattr(layer.self_attn.config, name, val)
            if method == "headkv":
                layer.self_attn.config.head_capacity = [[8] * 4] * 2
        with torch.no_grad():
            logits = model(torch.randint(0, 128, (1, L), generator=torch.Generator().manual_seed(1)), past_key_values=cache,
                           use_cache=True).logits
            for _ in range(steps):
                logits = model(logits[:, -1:].argmax(-1), past_key_values=cache, use_cache=True).logits
    finally:
        mp.replace_llama("fullkv")
    return model


@pytest.mark.parametrize("method", ["h2o", "cam", "l2norm", "adakv", "headkv", "think"])
def test_methods_without_a_decode_rule_refuse_the_cache(method):
    from kvcache_factory_amd import DecodeCompressedCache
    cache = DecodeCompressedCache(_config())
    layers = list(cache.layers)
    with pytest.raises(NotImplementedError, match=method) as e:
        _run_model(method, cache)
    assert "DecodeCompressedCache" in str(e.value)
    assert all(a is b for a, b in zip(cache.layers, layers)) and all(x.get_seq_length() == 0 for x in cache.layers)


def test_pivot_merge_and_fullkv_refuse_the_cache():
    from kvcache_factory_amd import DecodeCompressedCache
    with pytest.raises(NotImplementedError, match="snapkv with merge='pivot'"):
        _run_model("snapkv", DecodeCompressedCache(_config()), merge="pivot")
    with pytest.raises(NotImplementedError, match="fullkv"):
        _run_model("fullkv", DecodeCompressedCache(_config()))


def test_interval_below_window_raises_at_the_first_decode_forward():
    from kvcache_factory_amd import DecodeCompressedCache
    cache = DecodeCompressedCache(_config(), interval=4)
    with pytest.raises(ValueError, match="interval 4 must be >= window_size 8"):
        _run_model("snapkv", cache, L=20, steps=1)                # a pass-through prompt: the prefill needs no kernel
    assert cache.layers[0].get_seq_length() == 21                 # the prefill and the first decode step went through


# ---- layer bookkeeping with CPU stand-ins ----------------------------------------------------------------------------------
CALLS = []


def standin_decode_compress(method, ring, ring_start, kp, vp, P, kt, vt, T, out, W, n_keep, kernel_size=5, pooling="avgpool",
                            tie_mode="torch_cpu", return_indices=False, return_scores=False):
    """_kvc.decode_compress restated: the oracle's kvc_compress on the materialised cat(prefix, repeat_kv(tail))."""
    kb, vb = out
    hq, S = kb.shape[1], P + T
    G = hq // kt.shape[1]
    K = torch.cat([kp[:, :, :P], kt[:, :, :T].repeat_interleave(G, 1)], 2)
    V = torch.cat([vp[:, :, :P], vt[:, :, :T].repeat_interleave(G, 1)], 2)
    q = None
    if method != _kvc.STREAMINGLLM:
        q = torch.zeros(1, hq, S, K.shape[3], dtype=K.dtype)
        q[:, :, S - W:] = torch.roll(ring, -ring_start, dims=2)
    ko, vo = oracle_compress(method, q, K, V, W, n_keep, kernel_size, pooling, tie_mode, n_q_heads=hq)
    CALLS.append(dict(P=P, T=T, window=None if q is None else q[:, :, S - W:].clone(), K=K, V=V))
    assert not any(x.data_ptr() == kb.data_ptr() for x in (kp, vp, kt, vt))      # the output never aliases the input
    kb[:, :, :n_keep + W].copy_(ko)
    vb[:, :, :n_keep + W].copy_(vo)
    return kb[:, :, :n_keep + W], vb[:, :, :n_keep + W]


@pytest.fixture()
def cpu_kernels(monkeypatch):
    monkeypatch.setattr(_kvc, "decode_compress", standin_decode_compress)
    monkeypatch.setattr(_kvc, "decode_step", oracle_decode_step)
    monkeypatch.setattr(_kvc, "compress", oracle_compress)
    monkeypatch.setattr(_kvc, "compress_batch", oracle_compress_batch)
    CALLS.clear()
    yield


def _bf(g, *sh):
    return torch.randn(*sh, generator=g).to(torch.bfloat16)


def _drive(layer, cluster, g, sizes, form="split", hq=4, hkv=2, D=64):
    """Decode steps of `sizes` rows; returns per step (rows before, rows after the step's hook, compressed?) and the queries of
    every row."""
    log, qs = [], []
    for t in sizes:
        q, k, v = _bf(g, 1, hq, t, D), _bf(g, 1, hkv, t, D), _bf(g, 1, hkv, t, D)
        before, n0 = layer.stored_length(), layer.compressions
        if form == "split":
            layer.decode_attend(q, k, v, D ** -0.5)
        else:
            layer.update(k.repeat_interleave(hq // hkv, 1), v.repeat_interleave(hq // hkv, 1))
        qs.append(q)
        layer.after_decode(cluster, q)
        log.append((before, layer.stored_length(), layer.compressions > n0))
        assert layer.get_mask_sizes(1) == (layer.stored_length() + 1, 0)
    return log, torch.cat(qs, 2)


def _prefilled(g, P0, interval, hq=4, D=64):
    from kvcache_factory_amd import DecodeCompressedLayer
    layer = DecodeCompressedLayer(interval)
    layer.prefill(_bf(g, 1, hq, P0, D), _bf(g, 1, hq, P0, D), 1000)
    return layer


@pytest.mark.parametrize("form", ["split", "expanded"])
@pytest.mark.parametrize("method", ["snapkv", "streamingllm"])
def test_trigger_steps_lengths_and_ring(cpu_kernels, form, method):
    from kvcache_factory_amd import pyramidkv_utils as pu
    cl = (pu.SnapKVCluster(window_size=8, max_capacity_prompt=40, kernel_size=7, pooling="maxpool") if method == "snapkv"
          else pu.StreamingLLMKVCluster(window_size=8, max_capacity_prompt=40))
    g = torch.Generator().manual_seed(3)
    B, interval, W = 40, 16, 8
    layer = _prefilled(g, B, interval)
    sizes = [1] * 14 + [5, 1, 1, 3, 7, 1, 2] + [1] * 20 + [4, 4, 4] + [1] * 9
    log, qs = _drive(layer, cl, g, sizes, form)
    S, T, n, seen = B, 0, 0, 0
    for (before, after, comp), t in zip(log, sizes):
        assert before == S
        S, T, seen = S + t, T + t, seen + t
        expect = S >= B + interval and T >= W
        assert comp == expect, (S, T)
        if expect:
            call = CALLS[n] if form == "split" else None
            if call is not None:
                assert (call["P"], call["T"]) == (S - T, T)
                if method == "snapkv":                               # the ring's slots in chronological order = the last W queries
                    assert torch.equal(call["window"], qs[:, :, seen - W:seen])
            n += 1
            S, T = B, 0
            assert after == B
        assert after == S and before + t <= B + interval + t - 1
    assert n >= 4 and layer.compressions == n
    assert layer.get_seq_length() == 1000 + sum(sizes)
    if form == "split":
        assert len(CALLS) == n
    assert (layer._qring is None) == (method == "streamingllm")


def test_compression_result_is_the_rule_on_the_materialised_cache(cpu_kernels):
    """One compression step by step: the new prefix is what kvc_compress keeps of cat(prefix, repeat_kv(tail)) scored by the last W
    decoded rows' queries, in the other prefix buffer; the tail buffer is kept."""
    from kvcache_factory_amd import pyramidkv_utils as pu
    cl = pu.SnapKVCluster(window_size=8, max_capacity_prompt=40, kernel_size=7, pooling="maxpool")
    g = torch.Generator().manual_seed(5)
    layer = _prefilled(g, 40, 16)
    _drive(layer, cl, g, [1] * 15)
    K0, V0 = layer.keys.clone(), layer.values.clone()
    kbuf, tail = layer._kbuf, layer._ktail
    _, qs = _drive(layer, cl, g, [1])
    assert layer.compressions == 1
    K, V = layer.keys, layer.values
    call = CALLS[0]
    assert torch.equal(call["K"][:, :, :55], K0) and torch.equal(call["V"][:, :, :55], V0)
    q = torch.zeros(1, 4, 56, 64, dtype=torch.bfloat16)
    q[:, :, 48:] = call["window"]
    ko, vo = oracle_compress(_kvc.SNAPKV, q, call["K"], call["V"], 8, 32, 7, "maxpool", n_q_heads=4)
    assert torch.equal(K, ko) and torch.equal(V, vo)
    # the prefill's buffer (40 + RESERVE rows) is dropped, not kept as the alternate; the new prefix has exactly B rows
    assert layer._kbuf is not kbuf and layer._kalt is None and layer._ktail is tail
    first = layer._kbuf
    assert first.shape[2] == 40 and first.untyped_storage().nbytes() == first.numel() * first.element_size()
    _drive(layer, cl, g, [1] * 16)
    assert layer.compressions == 2 and layer._kalt is first and layer._kbuf.shape[2] == 40
    second = layer._kbuf
    _drive(layer, cl, g, [1] * 16)                                    # from here on the two B-row buffers alternate
    assert layer.compressions == 3 and layer._kbuf is first and layer._kalt is second
    _drive(layer, cl, g, [1] * 16)
    assert layer.compressions == 4 and layer._kbuf is second and layer._kalt is first


@pytest.mark.parametrize("method", ["snapkv", "streamingllm"])
def test_expanded_form_is_exact_whatever_the_dot_mode(cpu_kernels, monkeypatch, method):
    """KVC_DOT_MODE = mfma16 (the tolerance mode of prefill scoring) does not apply at decode time: the EXPANDED form's
    kvc_compress_batch call pins dot_mode EXACT, as kvc_decode_compress always computes."""
    from kvcache_factory_amd import pyramidkv_utils as pu
    monkeypatch.setattr(_kvc, "DOT_MODE", "mfma16")
    seen = []

    def spy(*a, dot_mode=None, **kw):
        seen.append(dot_mode)
        return oracle_compress_batch(*a, dot_mode=dot_mode, **kw)
    monkeypatch.setattr(_kvc, "compress_batch", spy)
    cl = (pu.SnapKVCluster(window_size=8, max_capacity_prompt=40, kernel_size=7, pooling="maxpool") if method == "snapkv"
          else pu.StreamingLLMKVCluster(window_size=8, max_capacity_prompt=40))
    g = torch.Generator().manual_seed(11)
    layer = _prefilled(g, 40, 16)
    _drive(layer, cl, g, [1] * 40, form="expanded")
    assert layer.compressions == 2 and seen == ["exact", "exact"]


def test_pyramidkv_budgets_and_a_prefill_above_the_budget(cpu_kernels):
    from kvcache_factory_amd import DecodeCompressedLayer, pyramidkv_utils as pu
    n_layers, cap, W = 6, 64, 8
    for li in range(n_layers):
        cl = pu.PyramidKVCluster(num_hidden_layers=n_layers, window_size=W, max_capacity_prompt=cap, layer_idx=li)
        _, B, w = DecodeCompressedLayer(16).budget(cl)
        assert w == W and B == _kvc.pyramid_k(cap, W, 2 * cap, li, n_layers) + W
        for q_len in (2 * cap, 5000):                                  # the per-layer branch: independent of the prompt length
            assert B == _kvc.pyramid_k(cap, W, q_len, li, n_layers) + W
    cl = pu.PyramidKVCluster(num_hidden_layers=n_layers, window_size=W, max_capacity_prompt=cap, layer_idx=n_layers - 1)
    B = DecodeCompressedLayer(16).budget(cl)[1]
    g = torch.Generator().manual_seed(7)
    layer = _prefilled(g, 100, 16)                                     # the short-prompt branch kept more than B rows
    assert 100 > B + 16
    log, qs = _drive(layer, cl, g, [1] * 7 + [1] + [1] * 30)
    assert [c for _, _, c in log][:8] == [False] * 7 + [True]         # first step with T >= W
    assert CALLS[0]["P"] == 100 and CALLS[0]["T"] == 8
    assert torch.equal(CALLS[0]["window"], qs[:, :, :8])
    assert layer.compressions >= 2 and layer.stored_length() <= B + 16


def test_beam_reordering_covers_the_new_state(cpu_kernels):
    from kvcache_factory_amd import DecodeCompressedLayer
    layer = DecodeCompressedLayer(16)
    g = torch.Generator().manual_seed(9)
    layer.prefill(_bf(g, 3, 4, 20, 64), _bf(g, 3, 4, 20, 64), 20)
    layer._kalt, layer._valt, layer._qring = _bf(g, 3, 4, 30, 64), _bf(g, 3, 4, 30, 64), _bf(g, 3, 4, 8, 64)
    bits = lambda t: t.view(torch.int16)                              # (the spare rows of _kbuf are uninitialised)
    before = {n: bits(getattr(layer, n)).clone() for n in ("_kalt", "_valt", "_qring", "_kbuf")}
    beam = torch.tensor([2, 0, 0])
    layer.reorder_cache(beam)
    for n, t in before.items():
        assert torch.equal(bits(getattr(layer, n)), t[beam]), n
    assert {"_kalt", "_valt", "_qring"} <= set(layer._batch_tensors)


def test_patched_model_generates_with_bounded_layers(cpu_kernels):
    """SnapKV on a tiny CPU Llama (the reference-shaped EXPANDED path): pass-through prompt, then compressions every interval."""
    from kvcache_factory_amd import DecodeCompressedCache
    cache = DecodeCompressedCache(_config(), interval=8)
    _run_model("snapkv", cache, L=20, steps=40, cap=24, W=8)
    for layer in cache.layers:
        assert layer.compressions >= 3 and not layer._split
        assert layer.get_seq_length() == 60 and layer.stored_length() < 24 + 8
        assert layer.get_mask_sizes(1)[0] == layer.stored_length() + 1
