"""Graph-replayed decoding without a GPU: the device-counted decode entry is declared, exported and checks its arguments before any
launch; its split plan depends on the bound alone (restated here); the layer's device-length mode and GraphDecoder's host
arithmetic — grow points, the mirrors after n steps, leaving the mode, the refusals — on a tiny Llama with the kernel call
replaced by an fp32 restatement (capture=False: a CPU has no graphs, the books are the same)."""
import ctypes
import os
import re

import pytest
import torch

from kvcache_factory_amd import _kvc
from test_batch_generation_cpu import _Patched, _config, _pad_left, _prompts, cpu_kernels, restated_decode_step_rows  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kvc_decode_dev_workspace_bytes", "kvc_decode_step_dev")


# ---- the plan, restated ---------------------------------------------------------------------------------------------------------
def dev_split_plan(bsz, hq, t, prefix_rows, tail_capacity):
    """(splits, rows_per_split) of kvc_decode_step_dev with a full workspace (kvc_decode_dev.hip: decode_dev_splits and
    launch_decode_step_dev): the plan of the BOUND prefix_rows + tail_capacity — kvc_decode_step2's target of 1024 workgroups for one
    sequence, kvc_decode_step_rows' 2048 for a batch; at least 64 rows per split, at most 64 splits, whole multiples of 64 rows."""
    rows = prefix_rows + tail_capacity
    heads = bsz * hq * t
    s = max(1, min(-(-(2048 if bsz > 1 else 1024) // heads), -(-rows // 64), 64))
    if s == 1:
        return 1, rows
    rps = -(-(-(-rows // s)) // 64) * 64
    return -(-rows // rps), rps


def visible_edges(bsz, hq, t, prefix_rows, tail_capacity):
    """Tail lengths T at which the LAST token's visible rows prefix_rows + T + t sit one below, at and one above every split boundary,
    plus the two ends — the values at which the number of splits that run changes."""
    splits, rps = dev_split_plan(bsz, hq, t, prefix_rows, tail_capacity)
    out = {0, tail_capacity - t}
    for s in range(1, splits):
        for vis in (s * rps - 1, s * rps, s * rps + 1):
            T = vis - prefix_rows - t
            if 0 <= T <= tail_capacity - t:
                out.add(T)
    return sorted(out)


def restated_decode_step_dev(q, k_new, v_new, k_prefix, v_prefix, prefix_rows, k_tail, v_tail, tail_counter, scaling, rows_b=None,
                             ws=None, out=None):
    """_kvc.decode_step_dev restated: the counter is clamped to [0, capacity - t], then the per-row step at that length."""
    b, _, t, _ = q.shape
    T = min(max(int(tail_counter.reshape(-1)[0]), 0), k_tail.shape[2] - t)
    rows = rows_b if rows_b is not None else torch.full((b,), prefix_rows, dtype=torch.int32)
    o = restated_decode_step_rows(q, k_new, v_new, k_prefix, v_prefix, rows, prefix_rows, k_tail, v_tail, T, scaling)
    if out is not None:
        out.copy_(o)
        return out
    return o


def _dp(kvc, **kw):
    p = kvc.DecodeParams()
    d = dict(dtype=kvc.BF16, bsz=1, n_q_heads=8, n_kv_heads=2, head_dim=128, prefix_rows=40, tail_rows=0, new_rows=1, scaling=0.1,
             q_stride_b=1024, q_stride_h=128, q_stride_l=128, new_stride_b=256, new_stride_h=128, new_stride_l=128,
             prefix_stride_b=8 * 48 * 128, prefix_stride_h=48 * 128, tail_stride_b=2 * 216 * 128, tail_stride_h=216 * 128,
             out_stride_b=1024, out_stride_h=128, out_stride_l=1024)
    d.update(kw)
    for k, v in d.items():
        setattr(p, k, v)
    return p


# ---- 1. declared, exported ---------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_exports_the_entry(kvc):
    header = open(os.path.join(ROOT, "include", "kvc.h")).read()
    L = kvc.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header) and name in kvc.EXPORTS
        getattr(L, name)
    assert L.kvc_version() == 5 == int(re.search(r"#define\s+KVC_VERSION\s+(\d+)", header).group(1))
    assert "tail_rows_dev" in header and "clamp(*tail_rows_dev, 0, tail_capacity - new_rows)" in header


# ---- 2. argument checks: an error text and no launch (no GPU here: a launch would fail differently) ----------------------------------
@pytest.mark.parametrize("kw,cap,code,msg", [
    (dict(new_rows=3), 2, -1, b"tail_capacity"),
    (dict(), 0, -1, b"tail_capacity"),
    (dict(), -7, -1, b"tail_capacity"),
    (dict(head_dim=96), 216, -2, b"head_dim"),
    (dict(dtype=7), 216, -1, b"dtype"),
    (dict(n_q_heads=7), 216, -1, b"head counts"),
    (dict(new_rows=0), 216, -1, b"row counts"),
    (dict(prefix_rows=-1), 216, -1, b"row counts"),
    (dict(prefix_rows=2 ** 31 - 100), 216, -1, b"overflows"),
])
def test_entry_rejects_invalid_params_before_any_pointer(kvc, kw, cap, code, msg):
    L = kvc.lib()
    a = ctypes.c_void_p(4096)                                               # never dereferenced
    p = _dp(kvc, **kw)
    assert L.kvc_decode_step_dev(ctypes.byref(p), cap, *([a] * 10), None, 0, None) == code
    assert msg in L.kvc_last_error(), L.kvc_last_error()
    assert L.kvc_decode_dev_workspace_bytes(ctypes.byref(p), cap) == 0 and msg in L.kvc_last_error()


def test_entry_rejects_null_and_misaligned_pointers(kvc):
    L = kvc.lib()
    a, odd, odd4 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8), ctypes.c_void_p(4096 + 2)
    p = _dp(kvc)
    assert L.kvc_decode_step_dev(None, 216, *([a] * 10), None, 0, None) == -1 and b"NULL" in L.kvc_last_error()
    assert L.kvc_decode_dev_workspace_bytes(None, 216) == 0
    assert L.kvc_decode_step_dev(ctypes.byref(p), 216, None, *([a] * 9), None, 0, None) == -1 and b"tail_rows_dev" in L.kvc_last_error()
    assert L.kvc_decode_step_dev(ctypes.byref(p), 216, odd4, *([a] * 9), None, 0, None) == -4 and b"tail_rows_dev" in L.kvc_last_error()
    assert L.kvc_decode_step_dev(ctypes.byref(p), 216, a, odd4, *([a] * 8), None, 0, None) == -4 and b"prefix_rows_b" in L.kvc_last_error()
    for hole in range(8):                                                    # q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, out
        args = [a] * 8
        args[hole] = None
        assert L.kvc_decode_step_dev(ctypes.byref(p), 216, a, None, *args, None, 0, None) == -1 and b"non-NULL" in L.kvc_last_error(), hole
        args[hole] = odd
        assert L.kvc_decode_step_dev(ctypes.byref(p), 216, a, None, *args, None, 0, None) == -4 and b"aligned" in L.kvc_last_error(), hole
    assert L.kvc_decode_step_dev(ctypes.byref(p), 216, a, None, *([a] * 8), odd, 1 << 20, None) == -4 and b"aligned" in L.kvc_last_error()
    assert L.kvc_decode_step_dev(ctypes.byref(_dp(kvc, tail_stride_h=216 * 128 + 4)), 216, a, None, *([a] * 8), None, 0, None) == -4
    # an empty prefix needs no prefix pointers; p->tail_rows is ignored, whatever it holds
    for kw in (dict(prefix_rows=0), dict(tail_rows=-9), dict(tail_rows=10 ** 9)):
        assert L.kvc_decode_dev_workspace_bytes(ctypes.byref(_dp(kvc, **kw)), 216) > 0, kw


# ---- 3. the plan depends on the bound alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bsz,hq,t,D,P,cap", [(1, 8, 1, 128, 40, 216), (1, 8, 3, 64, 40, 216), (3, 8, 1, 128, 40, 216), (1, 32, 1, 128, 136, 64),
                                              (1, 32, 1, 128, 2056, 1024), (1, 32, 1, 128, 2056, 8192), (8, 32, 1, 128, 520, 256),
                                              (1, 4, 1, 64, 0, 1), (1, 4, 5, 64, 7, 5), (2, 4, 1, 64, 16, 64), (1, 2, 1, 64, 9000, 4096)])
def test_workspace_and_plan_follow_the_bound_only(kvc, bsz, hq, t, D, P, cap):
    L = kvc.lib()
    splits, rps = dev_split_plan(bsz, hq, t, P, cap)
    assert splits == 1 or (rps % 64 == 0 and (splits - 1) * rps < P + cap <= splits * rps)
    want = 0 if splits == 1 else bsz * hq * t * _raw_splits(bsz, hq, t, P + cap) * (D + 2) * 4
    seen = set()
    for tail_rows in (0, 1, cap - t, cap + 1000, -3):                        # the host's idea of the tail changes nothing
        p = _dp(kvc, bsz=bsz, n_q_heads=hq, n_kv_heads=hq // 2, head_dim=D, prefix_rows=P, new_rows=t, tail_rows=tail_rows)
        seen.add(L.kvc_decode_dev_workspace_bytes(ctypes.byref(p), cap))
    assert seen == {want}


def _raw_splits(bsz, hq, t, rows):
    return max(1, min(-(-(2048 if bsz > 1 else 1024) // (bsz * hq * t)), -(-rows // 64), 64))


def test_issue_setup_gives_four_splits_of_64_rows_and_its_edges():
    assert dev_split_plan(1, 8, 1, 40, 216) == (4, 64) and dev_split_plan(3, 8, 1, 40, 216) == (4, 64)
    assert visible_edges(1, 8, 1, 40, 216) == [0, 22, 23, 24, 86, 87, 88, 150, 151, 152, 215]
    assert [40 + T + 1 for T in (0, 22, 23, 24, 87, 88, 215)] == [41, 63, 64, 65, 128, 129, 256]
    assert visible_edges(1, 8, 3, 40, 216)[-1] == 213


# ---- 4. the layer's device-length mode -------------------------------------------------------------------------------------------------
@pytest.fixture()
def dev_kernel(cpu_kernels, monkeypatch):
    calls = []

    def spy(*a, **kw):
        calls.append((int(a[8][0]), a[6].shape[2], kw.get("ws")))
        return restated_decode_step_dev(*a, **kw)
    monkeypatch.setattr(_kvc, "decode_step_dev", spy, raising=False)
    yield calls


def _layer(P=12, hq=4, D=64, seed=0):
    from kvcache_factory_amd.cache import CompressedDynamicLayer
    g = torch.Generator().manual_seed(seed)
    layer = CompressedDynamicLayer()
    layer.prefill(torch.randn(1, hq, P, D, generator=g).to(torch.bfloat16), torch.randn(1, hq, P, D, generator=g).to(torch.bfloat16), 100)
    return layer, g


def _qkv(g, t=1, hq=4, hkv=2, D=64):
    mk = lambda h: torch.randn(1, h, t, D, generator=g).to(torch.bfloat16)  # noqa: E731
    return mk(hq), mk(hkv), mk(hkv)


def test_layer_device_length_mode_books_growth_and_exit(dev_kernel, monkeypatch):
    monkeypatch.setattr(_kvc, "decode_step", lambda q, kn, vn, kp, vp, P, kt, vt, T, s: restated_decode_step_rows(
        q, kn, vn, kp, vp, torch.full((q.shape[0],), P, dtype=torch.int32), P, kt, vt, T, s))     # the same restatement, host-counted
    layer, g = _layer()
    plain, g2 = _layer()
    counter = torch.zeros(1, dtype=torch.int32)
    layer.enter_device_length(counter, 4, 2)
    assert layer._devlen and layer._split and layer.tail_capacity() == 4 and layer.stored_length() == 12 and layer.get_seq_length() == 100
    outs = []
    for n in range(9):
        if layer._tail + 1 > layer.tail_capacity():
            with pytest.raises(RuntimeError, match="grow_tail"):
                layer.decode_attend(*_qkv(torch.Generator().manual_seed(99)), 0.125)
            before = (layer._ktail[:, :, :layer._tail].clone(), layer._vtail[:, :, :layer._tail].clone())
            layer.grow_tail()
            assert torch.equal(layer._ktail[:, :, :layer._tail], before[0]) and torch.equal(layer._vtail[:, :, :layer._tail], before[1])
        q, k, v = _qkv(g)
        outs.append(layer.decode_attend(q, k, v, 0.125))
        counter.add_(1)
        assert layer._tail == n + 1 == int(counter) and layer.get_seq_length() == 101 + n and layer.stored_length() == 13 + n
        assert layer.get_mask_sizes(1) == (14 + n, 0) and layer.keys.shape == (1, 4, 13 + n, 64)
        assert int(layer.row_lengths()[0]) == 12
        ref = plain.decode_attend(*_qkv(g2), 0.125)                          # today's host-counted step on the same rows
        assert torch.equal(outs[-1].view(torch.int16), ref.view(torch.int16))
    assert [c[1] for c in dev_kernel] == [4] * 4 + [8] * 4 + [16]           # doubled at 4 and at 8 rows
    assert all(c[2] is not None and c[2].dtype == torch.uint8 for c in dev_kernel)      # its own workspace, never the pool
    assert len({c[2].data_ptr() for c in dev_kernel[:4]}) == 1              # one per capacity
    assert torch.equal(layer.keys.view(torch.int16), plain.keys.view(torch.int16))
    # held mirrors: the owner of a graph counts; leaving the mode (update) uses the mirror
    layer.hold_mirror(True)
    q, k, v = _qkv(g)
    layer.decode_attend(q, k, v, 0.125)
    assert layer._tail == 9 and layer.get_seq_length() == 109
    layer.advance(1)
    assert layer._tail == 10 and layer.get_seq_length() == 110
    k2, v2 = (torch.randn(1, 4, 1, 64, generator=g).to(torch.bfloat16) for _ in range(2))
    keys, _ = layer.update(k2, v2)
    assert not layer._devlen and not layer._split and layer._dev_counter is None and keys.shape == (1, 4, 23, 64)
    assert torch.equal(keys[:, :, 21].view(torch.int16), k.repeat_interleave(2, 1)[:, :, 0].view(torch.int16))
    assert layer.get_seq_length() == 111


def test_only_the_plain_layer_type_has_the_mode():
    from kvcache_factory_amd.cache import CompressedDynamicLayer, DecodeCompressedLayer, HeavyHitterLayer
    counter = torch.zeros(1, dtype=torch.int32)
    for cls in (DecodeCompressedLayer, HeavyHitterLayer):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls(8).enter_device_length(counter, 4, 2)
    with pytest.raises(RuntimeError, match="prefill"):
        CompressedDynamicLayer().enter_device_length(counter, 4, 2)


# ---- 5. GraphDecoder's host arithmetic ---------------------------------------------------------------------------------------------------
def test_tails_needed():
    from kvcache_factory_amd.graph_decode import tails_needed
    assert [tails_needed(4, T, 1) for T in (0, 3, 4, 7, 8, 16)] == [0, 0, 1, 1, 2, 3]
    assert tails_needed(1, 0, 1) == 0 and tails_needed(1, 1, 1) == 1 and tails_needed(32, 150, 1) == 3


@pytest.fixture()
def cpu_decoder(dev_kernel, monkeypatch):
    """The GPU-only gates opened for the stand-in kernels: the patched forward takes the fused step on CPU tensors."""
    from kvcache_factory_amd import attention, graph_decode
    real = attention._fusable
    monkeypatch.setattr(graph_decode, "_on_gpu", lambda t: True)
    monkeypatch.setattr(attention, "_fusable", lambda module, layer, h, m, kw: True if not h.is_cuda else real(module, layer, h, m, kw))
    yield dev_kernel


@pytest.mark.parametrize("method", ["snapkv", "pyramidkv", "streamingllm", "h2o"])
def test_decoder_grow_points_and_mirrors(cpu_decoder, method):
    from kvcache_factory_amd import GraphDecoder
    ids = _prompts((40,), seed=3)[0]
    with _Patched(method) as model:
        small, big = GraphDecoder(model, tail_rows=2, capture=False), GraphDecoder(model, tail_rows=64, capture=False)
        a = small.generate(ids, max_new_tokens=12)
        grows_at = []
        b_logits = [big.prefill(ids).clone()]
        s_logits = [small.prefill(ids).clone()]
        assert small.grows == 0 and int(small._counter) == 0 and small._pos.tolist() == [[40]]
        for j in range(11):
            tok = s_logits[-1][:, -1].argmax(-1, keepdim=True)
            g0 = small.grows
            s_logits.append(small.step(tok).clone())
            b_logits.append(big.step(tok).clone())
            if small.grows != g0:
                grows_at.append(j)
            for layer in small._cache.layers:
                assert layer._tail == j + 1 and layer.get_seq_length() == 41 + j and layer._devlen and layer._dev_counter is small._counter
                assert layer.tail_capacity() == small._capacity and layer.keys.shape[2] == layer._stored + j + 1
            assert int(small._counter) == j + 1 and small._pos.tolist() == [[41 + j]] and small._cache.get_seq_length() == 41 + j
        assert grows_at == [2, 4, 8] and small.grows == 3 and big.grows == 0 and small._capacity == 16   # full at 2, 4 and 8 rows
        for x, y in zip(s_logits, b_logits):                                 # the capacity and the growth change no byte
            assert torch.equal(x.view(torch.int16), y.view(torch.int16))
        toks = torch.cat([l[:, -1].argmax(-1, keepdim=True) for l in s_logits], 1)
        assert torch.equal(a[:, 40:], toks) and a.shape == (1, 52)
        for la, lb in zip(small._cache.layers, big._cache.layers):
            assert torch.equal(la.keys.view(torch.int16), lb.keys.view(torch.int16))
            assert torch.equal(la.values.view(torch.int16), lb.values.view(torch.int16))
    assert len(cpu_decoder) > 0 and all(c[2] is not None for c in cpu_decoder)


def test_decoder_batch_positions_follow_each_prompt(cpu_decoder):
    from kvcache_factory_amd import GraphDecoder
    prompts = _prompts((13, 40, 27), seed=4)
    ids, mask = _pad_left(prompts)
    with _Patched("snapkv") as model:
        dec = GraphDecoder(model, tail_rows=3, capture=False)
        out = dec.generate(ids, max_new_tokens=6, attention_mask=mask)
        assert dec._pos.tolist() == [[18], [45], [32]] and int(dec._counter) == 5 and dec.grows == 1
        layer = dec._cache.layers[0]
        assert layer.has_holes() and layer.row_lengths().tolist() == [13, 16, 16] and layer._tail == 5
        for b, p in enumerate(prompts):                                      # every row = that prompt decoded alone
            solo = GraphDecoder(model, tail_rows=3, capture=False).generate(p, max_new_tokens=6)
            assert torch.equal(out[b, 40:], solo[0, p.shape[1]:]), b


def test_decoder_refusals_raise_before_anything_is_stored(cpu_decoder, monkeypatch):
    from transformers import LlamaForCausalLM
    from kvcache_factory_amd import DecodeCompressedCache, GraphDecoder, HeavyHitterCache, KVQuantCompressedCache, QuantizedCompressedCache
    from kvcache_factory_amd import graph_decode, monkeypatch as mp, pyramidkv_utils as pu
    ids = _prompts((40,))[0]
    with pytest.raises(NotImplementedError, match="unpatched"):
        GraphDecoder(LlamaForCausalLM(_config()).eval().to(torch.bfloat16))
    for method in ("adakv", "headkv", "think"):
        with _Patched(method) as model:
            with pytest.raises(NotImplementedError, match=method):
                GraphDecoder(model)
    with _Patched("snapkv") as model:
        for cache, name in ((QuantizedCompressedCache(_config(), nbits=4), "quantized"), (KVQuantCompressedCache(_config(), nbits=4), "quantized"),
                            (DecodeCompressedCache(_config(), interval=8), "DecodeCompressedCache"),
                            (HeavyHitterCache(_config(), interval=8), "HeavyHitterCache")):
            dec = GraphDecoder(model, tail_rows=4, capture=False)
            with pytest.raises(NotImplementedError, match=name):
                dec.prefill(ids, past_key_values=cache)
            assert dec._cache is None and all(layer.get_seq_length() == 0 for layer in cache.layers)
        dec = GraphDecoder(model, tail_rows=4, capture=False)
        monkeypatch.setattr(pu, "DECODE_KERNEL", False)
        with pytest.raises(NotImplementedError, match="KVC_DECODE_KERNEL=0"):
            dec.prefill(ids)
        monkeypatch.setattr(pu, "DECODE_KERNEL", True)
        monkeypatch.setattr(pu, "BATCH_DECODE", False)
        with pytest.raises(NotImplementedError, match="KVC_BATCH_DECODE=0"):
            dec.prefill(torch.cat([ids, ids]))
        dec.prefill(ids)                                                     # one sequence does not need it
        monkeypatch.setattr(pu, "BATCH_DECODE", True)
        monkeypatch.setattr(graph_decode, "_on_gpu", lambda t: t.is_cuda)
        dec = GraphDecoder(model, tail_rows=4, capture=False)
        with pytest.raises(NotImplementedError, match="GPU only"):
            dec.prefill(ids)
        assert dec._cache is None
        monkeypatch.setattr(graph_decode, "_on_gpu", lambda t: True)
        model.config.sliding_window = 32
        with pytest.raises(NotImplementedError, match="sliding"):
            GraphDecoder(model)
        model.config.sliding_window = None
        model.train()
        with pytest.raises(NotImplementedError, match="eval"):
            GraphDecoder(model)
        model.eval()
        with pytest.raises(RuntimeError, match="before prefill"):
            GraphDecoder(model).step(ids[:, :1])
        for bad in (0, -1, True, 2.5):
            with pytest.raises(ValueError, match="tail_rows"):
                GraphDecoder(model, tail_rows=bad)
    with _Patched("snapkv", attn="eager") as model:                          # (transformers takes output_attentions with eager only)
        model.config.output_attentions = True
        with pytest.raises(NotImplementedError, match="output_attentions"):
            GraphDecoder(model)
    with _Patched("snapkv") as model:                                        # a head size the kernels are not built for
        monkeypatch.setattr(model.model.layers[0].self_attn, "head_dim", 96)
        with pytest.raises(NotImplementedError, match="head_dim"):
            GraphDecoder(model)
    assert mp._ORIGINALS                                                     # (the patches were restored by _Patched)
