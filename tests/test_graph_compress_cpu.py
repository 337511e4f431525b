"""Decode-stage compression under graph-replayed decoding, without a GPU: kvc_decode_step_dev_ring is declared, exported and checks
its arguments before any launch; the fixed tail's capacity against a host simulation of the trigger; BoundedDeviceLayer driven beside
DecodeCompressedLayer on the same rows with the kernels replaced by the stand-ins of the existing files; GraphDecoder(model,
interval=N) with capture=False on a tiny patched Llama — the mirrors, the per-layer counters, the prefix-length words, the refusals."""
import ctypes
import os
import re

import pytest
import torch

from kvcache_factory_amd import _kvc
from test_batch_generation_cpu import _prompts, cpu_kernels as prefill_kernels  # noqa: F401
from test_decode_compress_cpu import CALLS, cpu_kernels, standin_decode_compress  # noqa: F401
from test_graph_decode_cpu import _dp, dev_split_plan, restated_decode_step_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "kvc_decode_step_dev_ring"


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- 1. header, binding, argument checks ------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_exports_the_entry(kvc):
    header = open(os.path.join(ROOT, "include", "kvc.h")).read()
    L = kvc.lib()
    assert re.search(r"\b%s\(" % NEW, header) and NEW in kvc.EXPORTS
    getattr(L, NEW)
    assert L.kvc_version() == 5 == int(re.search(r"#define\s+KVC_VERSION\s+(\d+)", header).group(1))
    assert "(T + i) % W" in header and "ring_start = T_end % W" in header
    assert callable(kvc.decode_step_dev_ring)


def _ring_call(L, p, cap=216, counter=4096, ring=8192, W=8, sb=8 * 8 * 128, sh=8 * 128, hole=None):
    a = ctypes.c_void_p(4096)                                               # never dereferenced
    ptrs = [a] * 8                                                          # q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, out
    if hole is not None:
        ptrs[hole] = None
    vp = lambda x: None if x is None else ctypes.c_void_p(x)                # noqa: E731
    return L.kvc_decode_step_dev_ring(ctypes.byref(p), cap, vp(counter), None, *ptrs, vp(ring), W, sb, sh, None, 0, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(W=0), b"ring_rows"), (dict(W=-3), b"ring_rows"),
    (dict(ring=None), b"q_ring is NULL"),
    (dict(ring=8192 + 8), b"aligned"), (dict(sh=8 * 128 + 4), b"aligned"), (dict(sb=8 * 8 * 128 + 4), b"aligned"),
    (dict(sh=7 * 128), b"ring strides"), (dict(sb=7 * 8 * 128), b"ring strides"),
    (dict(cap=0), b"tail_capacity"),
    (dict(counter=None), b"tail_rows_dev"),
])
def test_entry_rejects_invalid_ring_arguments_before_any_pointer(kvc, kw, msg):
    L = kvc.lib()
    assert _ring_call(L, _dp(kvc), **kw) == kvc.ERR_INVALID
    assert msg in L.kvc_last_error(), L.kvc_last_error()


def test_entry_keeps_every_check_of_the_ringless_entry(kvc):
    L = kvc.lib()
    assert _ring_call(L, _dp(kvc, new_rows=3), cap=2) == -1 and b"tail_capacity" in L.kvc_last_error()
    for kw, code, msg in ((dict(head_dim=96), -2, b"head_dim"), (dict(dtype=7), -1, b"dtype"), (dict(n_q_heads=7), -1, b"head counts"),
                          (dict(new_rows=0), -1, b"row counts"), (dict(prefix_rows=2 ** 31 - 100), -1, b"overflows"),
                          (dict(tail_stride_h=216 * 128 + 4), -4, b"stride")):
        assert _ring_call(L, _dp(kvc, **kw)) == code and msg in L.kvc_last_error(), kw
    assert L.kvc_decode_step_dev_ring(None, 216, *([ctypes.c_void_p(4096)] * 11), 8, 8192, 1024, None, 0, None) == -1
    for hole in range(8):
        assert _ring_call(L, _dp(kvc), hole=hole) == -1 and b"non-NULL" in L.kvc_last_error(), hole
    assert _ring_call(L, _dp(kvc), counter=4096 + 2) == -4 and b"tail_rows_dev" in L.kvc_last_error()


@pytest.mark.parametrize("P,cap", [(40, 24), (2048, 128), (136, 64)])
def test_workspace_and_plan_are_the_ringless_entry_s(kvc, P, cap):
    """The entry has no workspace function of its own: kvc_decode_dev_workspace_bytes (the bound's plan, restated in
    test_graph_decode_cpu.dev_split_plan) sizes it, and the binding asks it with the same arguments for both entries."""
    header = open(os.path.join(ROOT, "include", "kvc.h")).read()
    doc = header[header.index("/* kvc_decode_step_dev_ring:"):header.index("int kvc_decode_step_dev_ring(")]
    assert "kvc_decode_dev_workspace_bytes" in doc
    hq, D = 8, 128
    q, kn = torch.zeros(1, hq, 1, D, dtype=torch.bfloat16), torch.zeros(1, 2, 1, D, dtype=torch.bfloat16)
    kp, kt = torch.zeros(1, hq, P, D, dtype=torch.bfloat16), torch.zeros(1, 2, cap, D, dtype=torch.bfloat16)
    splits = dev_split_plan(1, hq, 1, P, cap)[0]
    raw = max(1, min(-(-1024 // hq), -(-(P + cap) // 64), 64))
    assert kvc.decode_dev_plan(q, kn, kp, P, kt)[1] == (0 if splits == 1 else hq * raw * (D + 2) * 4)


# ---- 2. the fixed tail's capacity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 8])
def test_tail_capacity_is_what_the_trigger_can_need(W):
    from kvcache_factory_amd.cache import bounded_tail_rows, decode_trigger
    B = 40
    for interval in (W, 2 * W, 16):
        for P0 in (B - 20, B, B + 5, B + interval):
            cap = bounded_tail_rows(P0, B, interval)
            P, T, at_trigger = P0, 0, []
            for _ in range(6 * (B + interval)):                               # one-token steps
                assert T + 1 <= cap, (P0, interval, T)                       # the step's row fits
                T += 1
                if decode_trigger(P, T, B, W, interval):
                    at_trigger.append(T)
                    P, T = B, 0
            assert len(at_trigger) >= 4 and max(at_trigger) == cap, (P0, interval, at_trigger)   # reached, never passed
            assert at_trigger[0] == max(W, B + interval - P0) and set(at_trigger[1:]) == {interval}


# ---- stand-ins for the device-counted steps ------------------------------------------------------------------------------------------
def restated_decode_step_dev_ring(q, kn, vn, kp, vp, P, kt, vt, counter, scaling, ring, rows_b=None, ws=None, out=None):
    """_kvc.decode_step_dev_ring restated: query row i to slot (T + i) % W for i >= t - W, then the ring-less step."""
    t, W = q.shape[2], ring.shape[2]
    T = min(max(int(counter.reshape(-1)[0]), 0), kt.shape[2] - t)
    for i in range(max(0, t - W), t):
        ring[:, :, (T + i) % W] = q[:, :, i]
    return restated_decode_step_dev(q, kn, vn, kp, vp, P, kt, vt, counter, scaling, rows_b=rows_b, ws=ws, out=out)


@pytest.fixture()
def dev_kernels(cpu_kernels, monkeypatch):  # noqa: F811
    monkeypatch.setattr(_kvc, "decode_step_dev", restated_decode_step_dev)
    monkeypatch.setattr(_kvc, "decode_step_dev_ring", restated_decode_step_dev_ring)
    yield


# ---- 3. the bounded layer beside the host-counted one -------------------------------------------------------------------------------
def _cluster(method, W=8, cap=40):
    from kvcache_factory_amd import pyramidkv_utils as pu
    if method == "snapkv":
        return pu.SnapKVCluster(window_size=W, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool")
    if method == "pyramidkv":
        return pu.PyramidKVCluster(num_hidden_layers=4, window_size=W, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool", layer_idx=1)
    return pu.StreamingLLMKVCluster(window_size=W, max_capacity_prompt=cap)


def _bf(g, *sh):
    return torch.randn(*sh, generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("dP", [-20, 0, 5])
@pytest.mark.parametrize("method", ["snapkv", "pyramidkv", "streamingllm"])
def test_bounded_layer_follows_the_host_counted_layer(dev_kernels, method, dP):
    from kvcache_factory_amd.cache import BoundedDeviceLayer, CompressedDynamicLayer, DecodeCompressedLayer, bounded_tail_rows, decode_budget
    hq, hkv, D, interval = 4, 2, 64, 16
    cl = _cluster(method)
    _, B, W = decode_budget(cl, interval)
    P0 = B + dP
    g = torch.Generator().manual_seed(3 + dP)
    k0, v0 = _bf(g, 1, hq, P0, D), _bf(g, 1, hq, P0, D)
    host, plain = DecodeCompressedLayer(interval), CompressedDynamicLayer()
    host.prefill(k0.clone(), v0.clone(), 1000)
    plain.prefill(k0.clone(), v0.clone(), 1000)
    counters = torch.full((3,), 77, dtype=torch.int32)
    layer = BoundedDeviceLayer.adopt(plain, cl, interval, counters[1:2], hkv)
    assert layer._ktail.shape == (1, hkv, bounded_tail_rows(P0, B, interval), D) and layer._kbuf.shape[2] == max(P0, B)
    assert layer._kout.shape == (1, hq, B, D) and (layer._qring is None) == (method == "streamingllm")
    assert counters.tolist() == [77, 0, 77] and int(layer._plen) == P0 and layer.get_seq_length() == 1000
    addresses = [t.data_ptr() for t in (layer._kbuf, layer._vbuf, layer._ktail, layer._vtail, layer._plen, layer._kout, layer._vout)]
    at = []
    for step in range(56):                                                # P0 = B - 20: compressions after steps 36 and 52
        q, k, v = _bf(g, 1, hq, 1, D), _bf(g, 1, hkv, 1, D), _bf(g, 1, hkv, 1, D)
        n0 = host.compressions
        host.decode_attend(q, k, v, D ** -0.5)
        host.after_decode(cl, q)
        layer.decode_attend(q, k, v, D ** -0.5)
        layer.after_decode(cl, q)                                            # nothing: the owner calls the trigger
        assert layer._tail == int(counters[1])                               # the mirror is held: the owner advances it
        counters[1:2].add_(1)
        layer.advance(1)
        did = layer.maybe_compress()
        assert did == (host.compressions > n0) and layer.compressions == host.compressions, step
        assert layer.stored_length() == host.stored_length() and layer.rows() == host.rows(), step
        assert layer.get_seq_length() == host.get_seq_length() == 1001 + step
        assert int(layer._plen) == layer._stored and int(counters[1]) == layer._tail and counters[0] == counters[2] == 77
        if did:
            at.append(step)
            assert layer.stored_length() == B
            assert torch.equal(_bits(layer.keys), _bits(host.keys)) and torch.equal(_bits(layer.values), _bits(host.values)), step
    assert len(at) >= 2 and at[0] == max(W, B + interval - P0) - 1 and at[1] - at[0] == interval
    assert torch.equal(_bits(layer.keys), _bits(host.keys)) and torch.equal(_bits(layer.values), _bits(host.values))
    assert addresses == [t.data_ptr() for t in (layer._kbuf, layer._vbuf, layer._ktail, layer._vtail, layer._plen, layer._kout, layer._vout)]


def test_bounded_layer_limits(dev_kernels):
    from kvcache_factory_amd.cache import BoundedDeviceLayer, CompressedDynamicLayer, DecodeCompressedLayer, HeavyHitterLayer
    g = torch.Generator().manual_seed(1)
    counter = torch.zeros(1, dtype=torch.int32)
    cl = _cluster("snapkv")

    def plain(b=1):
        x = CompressedDynamicLayer()
        x.prefill(_bf(g, b, 4, 40, 64), _bf(g, b, 4, 40, 64), 100)
        return x
    for cls in (DecodeCompressedLayer, HeavyHitterLayer, BoundedDeviceLayer):                # the existing mode is the plain layer's only
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls(8).enter_device_length(counter, 4, 2)
    with pytest.raises(NotImplementedError, match="bsz = 1"):
        BoundedDeviceLayer.adopt(plain(2), cl, 16, counter, 2)
    with pytest.raises(NotImplementedError, match="DecodeCompressedLayer"):
        BoundedDeviceLayer.adopt(DecodeCompressedLayer(16), cl, 16, counter, 2)
    with pytest.raises(ValueError, match="interval 4 must be >= window_size 8"):
        BoundedDeviceLayer.adopt(plain(), cl, 4, counter, 2)
    for bad in (0, -3, 1.5, True, None):
        with pytest.raises(ValueError, match="interval"):
            BoundedDeviceLayer(bad)
    layer = BoundedDeviceLayer.adopt(plain(), cl, 16, counter, 2)
    with pytest.raises(NotImplementedError, match="fixed buffers"):
        layer.update(_bf(g, 1, 4, 1, 64), _bf(g, 1, 4, 1, 64))
    with pytest.raises(NotImplementedError, match="fixed buffers"):
        layer.reorder_cache(torch.tensor([0]))
    with pytest.raises(NotImplementedError, match="one-token"):
        layer.decode_attend(_bf(g, 1, 4, 2, 64), _bf(g, 1, 2, 2, 64), _bf(g, 1, 2, 2, 64), 0.125)
    with pytest.raises(NotImplementedError, match="never grows"):
        layer.grow_tail()


# ---- 4. GraphDecoder(model, interval=N), capture=False -----------------------------------------------------------------------------------
N_LAYERS, CAP, WIN = 4, 16, 4


def _config(attn="sdpa"):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=256, intermediate_size=128, num_hidden_layers=N_LAYERS, num_attention_heads=4, num_key_value_heads=2,
                       head_dim=64, vocab_size=128, max_position_embeddings=2048, attn_implementation=attn)


class _Patched:
    """A tiny 4-layer bf16 Llama with the attention forwards of `method` (restored on exit)."""

    def __init__(self, method, merge=None):
        self.method, self.knobs = method, dict(window_size=WIN, max_capacity_prompt=CAP, kernel_size=7, pooling="maxpool", merge=merge)

    def __enter__(self):
        from transformers import LlamaForCausalLM
        from kvcache_factory_amd import monkeypatch as mp
        torch.manual_seed(0)
        model = LlamaForCausalLM(_config()).eval().to(torch.bfloat16)
        mp.replace_llama(self.method)
        for layer in model.model.layers:
            for name, val in self.knobs.items():
                setattr(layer.self_attn.config, name, val)
        return model

    def __exit__(self, *exc):
        from kvcache_factory_amd import monkeypatch as mp
        mp.replace_llama("fullkv")


@pytest.fixture()
def cpu_decoder(prefill_kernels, dev_kernels, monkeypatch):  # noqa: F811
    """The GPU-only gates opened for the stand-in kernels: the patched forward takes the fused step on CPU tensors."""
    from kvcache_factory_amd import attention, graph_decode
    real = attention._fusable
    monkeypatch.setattr(_kvc, "decode_compress", standin_decode_compress)
    monkeypatch.setattr(graph_decode, "_on_gpu", lambda t: True)
    monkeypatch.setattr(attention, "_fusable", lambda module, layer, h, m, kw: True if not h.is_cuda else real(module, layer, h, m, kw))
    yield


@pytest.mark.parametrize("method", ["snapkv", "pyramidkv", "streamingllm"])
def test_decoder_follows_the_schedule(cpu_decoder, method):
    from kvcache_factory_amd import GraphDecoder
    from kvcache_factory_amd.cache import BoundedDeviceLayer, bounded_tail_rows, decode_trigger
    # (PyramidKV: a prompt on the short branch keeps CAP rows in every layer while the budgets differ, so the first triggers do)
    interval, L, steps = 8, 20 if method == "pyramidkv" else 40, 45
    ids = _prompts((L,), seed=3)[0]
    with _Patched(method) as model:
        dec = GraphDecoder(model, interval=interval, capture=False)
        logits = dec.prefill(ids)
        layers = dec._cache.layers
        assert len(layers) == N_LAYERS and all(type(x) is BoundedDeviceLayer for x in layers) and tuple(layers) == dec._layers
        assert dec._counter.shape == (N_LAYERS,) and dec._counter.dtype == torch.int32 and dec._counter.tolist() == [0] * N_LAYERS
        plans = [x._plan for x in layers]
        books = [[x._stored, 0] for x in layers]                            # (P, T) restated on the host
        caps = [x.tail_capacity() for x in layers]
        assert caps == [bounded_tail_rows(p, B, interval) for (p, _), (_, B, _) in zip(books, plans)]
        if method == "pyramidkv":
            assert len({B for _, B, _ in plans}) > 1 and {p for p, _ in books} == {CAP}
        else:
            assert {B for _, B, _ in plans} == {CAP} and all(p == CAP for p, _ in books)
        fired = [[] for _ in layers]
        CALLS.clear()
        for j in range(steps):
            tok = logits[:, -1].argmax(-1, keepdim=True)
            logits = dec.step(tok)
            for i, (layer, (_, B, W)) in enumerate(zip(layers, plans)):
                books[i][1] += 1
                if decode_trigger(books[i][0], books[i][1], B, W, interval):
                    books[i] = [B, 0]
                    fired[i].append(j)
                assert [layer._stored, layer._tail] == books[i] and int(layer._plen) == books[i][0], (j, i)
                assert layer._dev_counter.data_ptr() == dec._counter[i:i + 1].data_ptr() and layer.compressions == len(fired[i])
                assert layer.get_seq_length() == L + 1 + j and layer.tail_capacity() == caps[i]
            assert dec._counter.tolist() == [t for _, t in books] and dec._pos.tolist() == [[L + 1 + j]]
            assert dec._cache.get_seq_length() == L + 1 + j
        assert dec.grows == 0 and dec.captures == 0 and all(len(f) >= 3 for f in fired)
        assert len(CALLS) == sum(len(f) for f in fired)
        if method == "pyramidkv":
            assert len({tuple(f) for f in fired}) > 1                        # layers compress on different steps
        else:
            assert len({tuple(f) for f in fired}) == 1
        out = GraphDecoder(model, interval=interval, capture=False).generate(ids, max_new_tokens=12)
        assert out.shape == (1, L + 12)


def test_decoder_refusals_raise_before_anything_is_stored(cpu_decoder):
    from transformers import DynamicCache
    from kvcache_factory_amd import DecodeCompressedCache, GraphDecoder
    ids = _prompts((40,))[0]
    for method in ("h2o", "l2norm", "cam"):
        with _Patched(method) as model:
            with pytest.raises(NotImplementedError, match=method):
                GraphDecoder(model, interval=8, capture=False)
            GraphDecoder(model, capture=False)                               # without interval: as before
    with _Patched("snapkv", merge="pivot") as model:
        with pytest.raises(NotImplementedError, match="pivot"):
            GraphDecoder(model, interval=8, capture=False)
    with _Patched("snapkv") as model:
        for bad in (0, -1, True, 2.5, "8"):
            with pytest.raises(ValueError, match="interval must be an int >= 1"):
                GraphDecoder(model, interval=bad)
        with pytest.raises(ValueError, match="interval 3 must be >= window_size 4"):
            GraphDecoder(model, interval=3)
        dec = GraphDecoder(model, interval=8, capture=False)
        with pytest.raises(NotImplementedError, match="one sequence"):
            dec.prefill(torch.cat([ids, ids]))
        assert dec._cache is None and dec._counter is None
        for interval in (None, 8):                                           # as today, with and without the keyword
            cache = DecodeCompressedCache(_config(), interval=8)
            dec = GraphDecoder(model, interval=interval, capture=False)
            with pytest.raises(NotImplementedError, match="DecodeCompressedCache"):
                dec.prefill(ids, past_key_values=cache)
            assert dec._cache is None and all(layer.get_seq_length() == 0 for layer in cache.layers)
        cache = DynamicCache(config=model.config)
        dec = GraphDecoder(model, interval=8, capture=False)
        with pytest.raises(ValueError, match="past_key_values must be None"):
            dec.prefill(ids, past_key_values=cache)
        assert dec._cache is None and cache.get_seq_length() == 0
        for block in model.model.layers:                                     # the knobs can change after the decoder was built
            block.self_attn.config.merge = "pivot"
        with pytest.raises(NotImplementedError, match="pivot"):
            dec.prefill(ids)
        assert dec._cache is None
