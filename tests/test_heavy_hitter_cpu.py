"""The heavy-hitter cache without a GPU: the two new C-ABI entries' parameter structs and argument checks (every field, null
pointers), HeavyHitterCache's arguments and refusals, and the layer's bookkeeping with the two kernels replaced by torch stand-ins
that restate the rules (heavy_hitter_ref): which steps evict, lengths, buffer alternation, pass-through prompts, steps of several
tokens, a second generation on a reset cache."""
import ctypes
import os
import re

import pytest
import torch

import heavy_hitter_ref as R
from kvcache_factory_amd import _kvc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kvc.h")


# ---- C-ABI: structs and exports ----------------------------------------------------------------------------------------------
def _header_fields(name):
    text = open(HEADER).read()
    head = "typedef struct %s {" % name
    body = text[text.index(head) + len(head):text.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in re.findall(r"(?:int(?:32|64)_t|float|kvc_decode_params)\s+([^;]+);", body):
        fields += [f.strip() for f in decl.split(",")]
    return fields


def test_param_structs_match_header_and_exports(kvc):
    assert _header_fields("kvc_decode_scored_params") == [f[0] for f in kvc.DecodeScoredParams._fields_]
    assert _header_fields("kvc_decode_params") == [f[0] for f in kvc.DecodeParams._fields_]      # the nested struct
    assert _header_fields("kvc_decode_evict_params") == [f[0] for f in kvc.DecodeEvictParams._fields_]
    assert ctypes.sizeof(kvc.DecodeScoredParams) == ctypes.sizeof(kvc.DecodeParams) + 4 * 8
    assert ctypes.sizeof(kvc.DecodeEvictParams) == 10 * 4 + 12 * 8
    new = {"kvc_decode_step_scored", "kvc_decode_scored_workspace_bytes", "kvc_decode_evict", "kvc_decode_evict_workspace_bytes"}
    assert new <= set(kvc.EXPORTS)
    L = kvc.lib()
    for n in new:
        getattr(L, n)
    assert L.kvc_version() == 5                                       # the ABI is additive


# ---- kvc_decode_step_scored argument checks ----------------------------------------------------------------------------------
def _sp(kvc, **kw):
    sp = kvc.DecodeScoredParams()
    base = dict(dtype=kvc.BF16, bsz=1, n_q_heads=32, n_kv_heads=8, head_dim=128, prefix_rows=2048, tail_rows=100, new_rows=1,
                scaling=128 ** -0.5, q_stride_b=32 * 128, q_stride_h=128, q_stride_l=128, new_stride_b=8 * 128, new_stride_h=128,
                new_stride_l=128, prefix_stride_b=32 * 2048 * 128, prefix_stride_h=2048 * 128, tail_stride_b=8 * 256 * 128,
                tail_stride_h=256 * 128, out_stride_b=32 * 128, out_stride_h=128, out_stride_l=32 * 128)
    score = dict(score_prefix_stride_b=32 * 2048, score_prefix_stride_h=2048, score_tail_stride_b=32 * 256, score_tail_stride_h=256)
    for k, v in {**base, **score, **kw}.items():
        setattr(sp if k in score else sp.step, k, v)
    return sp


SCORED_BAD = [
    (dict(dtype=3), -1, "dtype"), (dict(dtype=-1), -1, "dtype"), (dict(bsz=0), -1, "head counts"), (dict(n_q_heads=0), -1, "head counts"),
    (dict(n_kv_heads=0), -1, "head counts"), (dict(n_kv_heads=5), -1, "head counts"), (dict(head_dim=96), -2, "head_dim"),
    (dict(prefix_rows=-1), -1, "row counts"), (dict(tail_rows=-1), -1, "row counts"), (dict(new_rows=0), -1, "row counts"),
    (dict(prefix_rows=2 ** 31 - 50), -1, "overflows"),
    (dict(q_stride_h=4), -4, "stride"), (dict(q_stride_l=129), -4, "stride"), (dict(new_stride_b=3), -4, "stride"),
    (dict(prefix_stride_h=2048 * 128 + 1), -4, "stride"), (dict(tail_stride_b=7), -4, "stride"),
    (dict(score_prefix_stride_h=2047), -1, "score_prefix strides"), (dict(score_prefix_stride_b=31 * 2048), -1, "score_prefix strides"),
    (dict(score_tail_stride_h=100), -1, "score_tail strides"), (dict(score_tail_stride_b=31 * 256), -1, "score_tail strides"),
]


@pytest.mark.parametrize("kw,code,msg", SCORED_BAD, ids=[f"{list(b[0])[0]}={list(b[0].values())[0]}" for b in SCORED_BAD])
def test_scored_invalid_params_rejected_before_any_pointer(kvc, kw, code, msg):
    L = kvc.lib()
    rc = L.kvc_decode_step_scored(ctypes.byref(_sp(kvc, **kw)), *([None] * 11), 0, None)
    assert rc == code and msg in L.kvc_last_error().decode(), (rc, L.kvc_last_error())
    assert L.kvc_decode_scored_workspace_bytes(ctypes.byref(_sp(kvc, **kw))) == 0


def test_scored_null_pointers_alignment_and_workspace(kvc):
    L = kvc.lib()
    assert L.kvc_decode_step_scored(None, *([None] * 11), 0, None) == -1 and b"NULL" in L.kvc_last_error()
    assert L.kvc_decode_scored_workspace_bytes(None) == 0
    p = _sp(kvc)
    need = L.kvc_decode_scored_workspace_bytes(ctypes.byref(p))
    # the logits [32][1][2149] fp32 and (M, Lsum, acc[128]) of every split
    assert need >= 32 * 2149 * 4 + 32 * 130 * 4 and need % 16 == 0 and L.kvc_last_error() == b""
    a = ctypes.c_void_p(1 << 40)                                  # never dereferenced: every check comes first
    good = [a] * 10                                               # q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, sp, st, out
    for i in range(10):
        args = list(good)
        args[i] = None
        rc = L.kvc_decode_step_scored(ctypes.byref(p), *args, a, need, None)
        assert rc == -1 and b"non-NULL" in L.kvc_last_error(), i
    for i in range(7):
        args = list(good)
        args[i] = ctypes.c_void_p((1 << 40) + 8)
        assert L.kvc_decode_step_scored(ctypes.byref(p), *args, a, need, None) == -4 and b"16-byte" in L.kvc_last_error(), i
    for i in (7, 8):
        args = list(good)
        args[i] = ctypes.c_void_p((1 << 40) + 2)
        assert L.kvc_decode_step_scored(ctypes.byref(p), *args, a, need, None) == -4 and b"4-byte" in L.kvc_last_error(), i
    assert L.kvc_decode_step_scored(ctypes.byref(p), *good, None, 0, None) == -3 and b"NULL" in L.kvc_last_error()
    assert L.kvc_decode_step_scored(ctypes.byref(p), *good, ctypes.c_void_p((1 << 41) + 8), need, None) == -3
    assert L.kvc_decode_step_scored(ctypes.byref(p), *good, a, need - 16, None) == -3 and b"too small" in L.kvc_last_error()
    # no prefix rows: the prefix pointers and score_prefix may be NULL (the remaining checks still come before any use)
    p0 = _sp(kvc, prefix_rows=0)
    args = list(good)
    args[3] = args[4] = args[7] = None
    assert L.kvc_decode_step_scored(ctypes.byref(p0), *args, None, 0, None) == -3


# ---- kvc_decode_evict argument checks ----------------------------------------------------------------------------------------
def _ep(kvc, **kw):
    p = kvc.DecodeEvictParams()
    base = dict(dtype=kvc.BF16, bsz=1, n_q_heads=32, n_kv_heads=8, head_dim=128, prefix_rows=2048, tail_rows=128, window=32, k=2016,
                tie_mode=kvc.TIES_TORCH_CPU, prefix_stride_b=32 * 2048 * 128, prefix_stride_h=2048 * 128, tail_stride_b=8 * 256 * 128,
                tail_stride_h=256 * 128, out_stride_b=32 * 2048 * 128, out_stride_h=2048 * 128, score_prefix_stride_b=32 * 2048,
                score_prefix_stride_h=2048, score_tail_stride_b=32 * 256, score_tail_stride_h=256, score_out_stride_b=32 * 2048,
                score_out_stride_h=2048)
    base.update(kw)
    for k, v in base.items():
        setattr(p, k, v)
    return p


EVICT_BAD = [
    (dict(dtype=3), -1, "dtype"), (dict(bsz=0), -1, "positive"), (dict(n_q_heads=0), -1, "positive"), (dict(n_kv_heads=0), -1, "positive"),
    (dict(n_kv_heads=5), -1, "multiple"), (dict(head_dim=96), -2, "head_dim"), (dict(window=0), -1, "window"),
    (dict(prefix_rows=-1), -1, "prefix_rows"), (dict(tail_rows=31), -1, "tail_rows 31"), (dict(k=-1), -1, "k=-1"), (dict(k=2145), -1, "k=2145"),
    (dict(tie_mode=2), -1, "tie_mode"),
    (dict(tie_mode=1, prefix_rows=200000, k=16385, prefix_stride_h=200000 * 128, prefix_stride_b=32 * 200000 * 128,
          out_stride_h=16417 * 128, out_stride_b=32 * 16417 * 128), -2, "canonical"),
    (dict(prefix_rows=2000000, k=18001, prefix_stride_h=2000000 * 128, prefix_stride_b=32 * 2000000 * 128,
          out_stride_h=18033 * 128, out_stride_b=32 * 18033 * 128), -2, "partial_sort"),
    (dict(prefix_stride_b=3), -4, "prefix strides"), (dict(prefix_stride_h=2047 * 128), -1, "prefix strides"),
    (dict(tail_stride_h=127 * 128), -1, "tail strides"), (dict(tail_stride_b=7 * 256 * 128), -1, "tail strides"),
    (dict(out_stride_h=2047 * 128), -1, "out strides"), (dict(out_stride_b=4), -4, "out strides"),
    (dict(score_prefix_stride_h=2047), -1, "score_prefix strides"), (dict(score_prefix_stride_b=31 * 2048), -1, "score_prefix strides"),
    (dict(score_tail_stride_h=127), -1, "score_tail strides"), (dict(score_tail_stride_b=31 * 256), -1, "score_tail strides"),
    (dict(score_out_stride_h=2047), -1, "score_out strides"), (dict(score_out_stride_b=31 * 2048), -1, "score_out strides"),
]


@pytest.mark.parametrize("kw,code,msg", EVICT_BAD, ids=[f"{list(b[0])[0]}={list(b[0].values())[0]}" for b in EVICT_BAD])
def test_evict_invalid_params_rejected_before_any_pointer(kvc, kw, code, msg):
    L = kvc.lib()
    rc = L.kvc_decode_evict(ctypes.byref(_ep(kvc, **kw)), *([None] * 11), 0, None)
    assert rc == code and msg in L.kvc_last_error().decode(), (rc, L.kvc_last_error())
    assert L.kvc_decode_evict_workspace_bytes(ctypes.byref(_ep(kvc, **kw))) == 0


def test_evict_null_pointers_overlap_and_workspace(kvc):
    L = kvc.lib()
    assert L.kvc_decode_evict(None, *([None] * 11), 0, None) == -1 and b"NULL" in L.kvc_last_error()
    p = _ep(kvc)
    need = L.kvc_decode_evict_workspace_bytes(ctypes.byref(p))
    assert need >= 32 * 2144 * 4 + 32 * 2016 * 8 and need % 256 == 0 and L.kvc_last_error() == b""
    base = 1 << 40
    ptr = lambda off: ctypes.c_void_p(base + off)
    pre_b, tail_b, sc_b = 32 * 2048 * 128 * 2, 8 * 256 * 128 * 2, 32 * 2048 * 4
    kp, vp, kt, vt = 0, pre_b, 2 * pre_b, 2 * pre_b + tail_b
    free = 2 * pre_b + 2 * tail_b
    sp, st, ko, vo, so = free, free + sc_b, free + 2 * sc_b, free + 2 * sc_b + pre_b, free + 2 * sc_b + 2 * pre_b
    good = [ptr(x) for x in (kp, vp, kt, vt, sp, st, ko, vo, so)]
    for i in range(9):
        args = list(good)
        args[i] = None
        rc = L.kvc_decode_evict(ctypes.byref(p), *args, None, ptr(1 << 35), need, None)
        assert rc == -1 and b"non-NULL" in L.kvc_last_error(), i
    for i in (0, 1, 2, 3, 6, 7):
        args = list(good)
        args[i] = ctypes.c_void_p(args[i].value + 8)
        assert L.kvc_decode_evict(ctypes.byref(p), *args, None, ptr(1 << 35), need, None) == -4 and b"16-byte" in L.kvc_last_error(), i
    for i in (4, 5, 8):
        args = list(good)
        args[i] = ctypes.c_void_p(args[i].value + 2)
        assert L.kvc_decode_evict(ctypes.byref(p), *args, None, ptr(1 << 35), need, None) == -4 and b"4-byte" in L.kvc_last_error(), i
    assert L.kvc_decode_evict(ctypes.byref(p), *good, ctypes.c_void_p(base + 8), ptr(1 << 35), need, None) == -4
    for i, off in ((6, kp), (7, vp + 4096), (6, kt), (7, ko + pre_b // 2), (6, vt - 4096), (8, sp), (8, st - 64)):
        args = list(good)
        args[i] = ptr(off)
        rc = L.kvc_decode_evict(ctypes.byref(p), *args, None, ptr(1 << 35), need, None)
        assert rc == -1 and b"overlap" in L.kvc_last_error(), (i, off)
    assert L.kvc_decode_evict(ctypes.byref(p), *good, None, None, 0, None) == -3
    assert L.kvc_decode_evict(ctypes.byref(p), *good, None, ptr(1 << 35 | 128), need, None) == -3
    assert L.kvc_decode_evict(ctypes.byref(p), *good, None, ptr(1 << 35), need - 256, None) == -3 and b"too small" in L.kvc_last_error()


# ---- the cache object and its refusals ---------------------------------------------------------------------------------------
def _config(layers=2):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=256, intermediate_size=128, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2,
                       head_dim=64, vocab_size=128, max_position_embeddings=2048, attn_implementation="sdpa")


def test_cache_arguments():
    from kvcache_factory_amd import HeavyHitterCache, HeavyHitterLayer
    from kvcache_factory_amd.cache import CompressedDynamicLayer
    c = HeavyHitterCache(_config(3), interval=64)
    assert len(c.layers) == 3 and all(isinstance(x, HeavyHitterLayer) for x in c.layers)
    assert issubclass(HeavyHitterLayer, CompressedDynamicLayer)
    assert c.interval == 64 and c.layers[0].interval == 64 and HeavyHitterCache(_config()).layers[1].interval == 128
    for bad in (0, -3, 1.5, True, "8", None):
        with pytest.raises(ValueError, match="interval"):
            HeavyHitterCache(_config(), interval=bad)
        with pytest.raises(ValueError, match="interval"):
            HeavyHitterLayer(bad)


def _run_model(method, cache, L=40, steps=1, merge=None, cap=64, W=8, bsz=1, **fwd):
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
            logits = model(torch.randint(0, 128, (bsz, L), generator=torch.Generator().manual_seed(1)), past_key_values=cache,
                           use_cache=True).logits
            for _ in range(steps):
                logits = model(logits[:, -1:].argmax(-1), past_key_values=cache, use_cache=True, **fwd).logits
    finally:
        mp.replace_llama("fullkv")
    return model


def _untouched(cache, layers):
    return all(a is b for a, b in zip(cache.layers, layers)) and all(x.get_seq_length() == 0 and x._kbuf is None for x in cache.layers)


@pytest.mark.parametrize("method", ["snapkv", "pyramidkv", "streamingllm", "cam", "l2norm", "adakv", "headkv", "think"])
def test_other_methods_refuse_the_cache(method):
    from kvcache_factory_amd import HeavyHitterCache
    cache = HeavyHitterCache(_config())
    layers = list(cache.layers)
    with pytest.raises(NotImplementedError, match=method) as e:
        _run_model(method, cache)
    assert "HeavyHitterCache" in str(e.value)
    assert _untouched(cache, layers)


def test_pivot_merge_fullkv_and_batches_refuse_the_cache():
    from kvcache_factory_amd import HeavyHitterCache
    for kw, pat in ((dict(method="h2o", merge="pivot"), "h2o with merge='pivot'"), (dict(method="fullkv"), "fullkv"),
                    (dict(method="h2o", bsz=2), "bsz = 1")):
        cache = HeavyHitterCache(_config())
        layers = list(cache.layers)
        with pytest.raises(NotImplementedError, match=pat) as e:
            _run_model(cache=cache, **kw)
        assert "HeavyHitterCache" in str(e.value)
        assert _untouched(cache, layers)
    layer = HeavyHitterCache(_config()).layers[0]
    layer.prefill(torch.zeros(1, 4, 20, 64), torch.zeros(1, 4, 20, 64), 20)
    for op, arg in ((layer.reorder_cache, torch.tensor([0])), (layer.batch_repeat_interleave, 2), (layer.batch_select_indices, torch.tensor([0]))):
        with pytest.raises(NotImplementedError, match="HeavyHitterCache"):
            op(arg)
    with pytest.raises(NotImplementedError, match="HeavyHitterCache"):
        HeavyHitterCache(_config()).layers[0].prefill(torch.zeros(2, 4, 20, 64), torch.zeros(2, 4, 20, 64), 20)


def test_a_step_the_fused_kernel_cannot_take_is_refused_with_the_cache_left_as_it_was(monkeypatch):
    """A pass-through prompt (no kernel at prefill), then a decode step on CPU tensors — what KVC_DECODE_KERNEL=0, output_attentions
    or bsz > 1 also lead to: the reference-shaped path, i.e. the layer's update().  It raises instead of dropping the scores."""
    from kvcache_factory_amd import HeavyHitterCache, pyramidkv_utils as pu
    for fwd, off in ((dict(), False), (dict(output_attentions=True), False), (dict(), True)):
        monkeypatch.setattr(pu, "DECODE_KERNEL", not off)
        cache = HeavyHitterCache(_config())
        with pytest.raises(NotImplementedError, match="HeavyHitterCache.*fused decode step"):
            _run_model("h2o", cache, L=20, steps=1, **fwd)
        for layer in cache.layers:                                   # the prefill went through, the refused step stored nothing
            assert layer.get_seq_length() == 20 and layer.stored_length() == 20 and layer.rows() == (20, 0)
            assert layer._ktail is None and float(layer.scores().abs().sum()) == 0.0


# ---- layer bookkeeping with torch stand-ins ----------------------------------------------------------------------------------
@pytest.fixture()
def cpu_kernels(monkeypatch):
    monkeypatch.setattr(_kvc, "decode_step_scored", R.standin_decode_step_scored)
    monkeypatch.setattr(_kvc, "decode_evict", R.standin_decode_evict)
    monkeypatch.setattr(_kvc, "compress", R.standin_compress)
    R.EVICTIONS.clear()
    yield


def _bf(g, *sh):
    return torch.randn(*sh, generator=g).to(torch.bfloat16)


def _cluster(cap=40, W=8, **kw):
    from kvcache_factory_amd import pyramidkv_utils as pu
    return pu.H2OKVCluster(window_size=W, max_capacity_prompt=cap, **kw)


def _prefilled(g, P0, interval, hq=4, D=64, scores=True):
    from kvcache_factory_amd import HeavyHitterLayer
    layer = HeavyHitterLayer(interval)
    layer.prefill(_bf(g, 1, hq, P0, D), _bf(g, 1, hq, P0, D), 1000)
    if scores:
        layer._sbuf[:, :, :P0] = torch.rand(1, hq, P0, generator=g) * 5
    return layer


def _drive(layer, cluster, g, sizes, hq=4, hkv=2, D=64):
    log = []
    for t in sizes:
        q, k, v = _bf(g, 1, hq, t, D) * 1.5, _bf(g, 1, hkv, t, D), _bf(g, 1, hkv, t, D)
        before, n0, s0 = layer.stored_length(), layer.evictions, layer.scores()
        out = layer.decode_attend(q, k, v, D ** -0.5)
        assert out.shape == (1, t, hq, D)
        s1 = layer.scores()
        inc = s1.clone()
        inc[:, :, :before] -= s0
        # every token adds a probability distribution: the step's increments sum to t per head
        assert torch.allclose(inc.sum(-1), torch.full((1, hq), float(t)), atol=1e-3)
        assert bool((inc[:, :, before:] >= 0).all())
        layer.after_decode(cluster, q)
        log.append((before, layer.stored_length(), layer.evictions > n0))
        assert layer.get_mask_sizes(1) == (layer.stored_length() + 1, 0) and layer.get_mask_sizes(3)[0] == layer.stored_length() + 3
    return log


def test_which_steps_evict_and_lengths(cpu_kernels):
    g = torch.Generator().manual_seed(3)
    B, interval, W = 40, 16, 8
    layer = _prefilled(g, B, interval)
    sizes = [1] * 14 + [5, 1, 1, 3, 7, 1, 2] + [1] * 20 + [4, 4, 4] + [1] * 9
    log = _drive(layer, _cluster(), g, sizes)
    S, T, n = B, 0, 0
    for (before, after, ev), t in zip(log, sizes):
        assert before == S
        S, T = S + t, T + t
        expect = S >= B + interval and T >= W
        assert ev == expect, (S, T)
        if expect:
            call = R.EVICTIONS[n]
            assert (call["P"], call["T"]) == (S - T, T)
            n += 1
            S, T = B, 0
        assert after == S and before + t <= B + interval + t - 1
    assert n >= 4 and layer.evictions == n == len(R.EVICTIONS)
    assert layer.get_seq_length() == 1000 + sum(sizes)


def test_eviction_result_is_the_rule_and_buffers_alternate(cpu_kernels):
    g = torch.Generator().manual_seed(5)
    layer = _prefilled(g, 40, 16)
    cl = _cluster()
    _drive(layer, cl, g, [1] * 15)
    K0, V0, s0, tail = layer.keys.clone(), layer.values.clone(), layer.scores(), layer._ktail
    assert s0.shape == (1, 4, 55) and layer._stail.shape[:2] == (1, 4)          # a tail row has one score per QUERY head
    first_buf = layer._kbuf
    _drive(layer, cl, g, [1])
    assert layer.evictions == 1 and layer.rows() == (40, 0)
    call = R.EVICTIONS[0]
    assert torch.equal(call["K"][:, :, :55], K0) and torch.equal(call["V"][:, :, :55], V0)
    assert torch.equal(call["score"][:, :, :55] >= s0, torch.ones_like(s0, dtype=torch.bool))   # the 16th step only added
    ko, vo, so, idx = R.evict_reference(call["K"], call["V"], call["score"], 8, 32, "torch_cpu")
    assert torch.equal(layer.keys, ko) and torch.equal(layer.values, vo) and torch.equal(layer.scores(), so)
    assert torch.equal(idx, torch.topk(call["score"][:, :, :48], 32).indices)
    # the prefill's buffer (40 + RESERVE rows) is dropped; the new prefix and its scores have exactly B rows; the tail is reused
    assert layer._kbuf is not first_buf and layer._kalt is None and layer._salt is None and layer._ktail is tail
    a = (layer._kbuf, layer._vbuf, layer._sbuf)
    assert a[0].shape[2] == 40 and a[2].shape == (1, 4, 40) and a[2].dtype == torch.float32
    _drive(layer, cl, g, [1] * 16)
    assert layer.evictions == 2 and (layer._kalt, layer._valt, layer._salt) == a
    b = (layer._kbuf, layer._vbuf, layer._sbuf)
    _drive(layer, cl, g, [1] * 16)                                    # from here on the two sets alternate
    assert layer.evictions == 3 and (layer._kbuf, layer._vbuf, layer._sbuf) == a and (layer._kalt, layer._valt, layer._salt) == b
    _drive(layer, cl, g, [1] * 16)
    assert layer.evictions == 4 and (layer._kbuf, layer._vbuf, layer._sbuf) == b


def test_prefill_scores_from_the_h2o_compression_and_pass_through(cpu_kernels):
    from kvcache_factory_amd import HeavyHitterLayer, pyramidkv_utils as pu
    from cpu_compress import oracle_compress
    g = torch.Generator().manual_seed(7)
    cl = _cluster(cap=24, W=8)
    q, k, v = _bf(g, 1, 4, 60, 64), _bf(g, 1, 2, 60, 64), _bf(g, 1, 2, 60, 64)
    layer = HeavyHitterLayer(8)
    pu.prefill_heavy_hitter(cl, layer, k, q, v)
    ko, vo, idx, sc = oracle_compress(_kvc.H2O, q, k, v, 8, 16, return_indices=True, return_scores=True)
    kc, vc = cl.update_kv(k, q, v, None, 2)                          # the H2O path itself, unchanged
    assert torch.equal(layer.keys, ko) and torch.equal(layer.keys, kc) and torch.equal(layer.values, vc)
    assert layer.rows() == (24, 0) and layer.get_seq_length() == 60 and layer._kbuf.shape[2] == 24      # exactly B rows
    s = layer.scores()
    assert s.dtype == torch.float32 and torch.equal(s[:, :, :16], sc.gather(2, idx).float()) and float(s[:, :, 16:].abs().sum()) == 0
    # a prompt below max_capacity_prompt: cached whole (expanded), every score 0; the first eviction waits for S >= B + interval
    layer = HeavyHitterLayer(8)
    pu.prefill_heavy_hitter(cl, layer, k[:, :, :20], q[:, :, :20], v[:, :, :20])
    assert layer.rows() == (20, 0) and torch.equal(layer.keys, k[:, :, :20].repeat_interleave(2, 1))
    assert float(layer.scores().abs().sum()) == 0
    log = _drive(layer, cl, g, [1] * 14)
    assert [e for _, _, e in log] == [False] * 11 + [True, False, False] and layer.stored_length() == 26
    assert R.EVICTIONS[-1]["P"] == 20 and R.EVICTIONS[-1]["T"] == 12


def test_interval_below_window_and_wrong_cluster(cpu_kernels):
    from kvcache_factory_amd import pyramidkv_utils as pu
    g = torch.Generator().manual_seed(9)
    layer = _prefilled(g, 40, 4)
    with pytest.raises(ValueError, match="interval 4 must be >= window_size 8"):
        _drive(layer, _cluster(), g, [1])
    layer = _prefilled(g, 40, 16)
    with pytest.raises(NotImplementedError, match="HeavyHitterCache.*SnapKVCluster"):
        _drive(layer, pu.SnapKVCluster(window_size=8, max_capacity_prompt=40), g, [1])
    with pytest.raises(NotImplementedError, match="merge='pivot'"):
        _drive(_prefilled(g, 40, 16), _cluster(merge="pivot"), g, [1])


def test_second_generation_on_a_reset_cache(cpu_kernels):
    from kvcache_factory_amd import HeavyHitterCache, pyramidkv_utils as pu
    cache = HeavyHitterCache(_config(), interval=8)
    cl = _cluster(cap=24, W=8)
    g = torch.Generator().manual_seed(11)
    for run in range(2):
        for layer in cache.layers:
            q, k, v = _bf(g, 1, 4, 50, 64), _bf(g, 1, 2, 50, 64), _bf(g, 1, 2, 50, 64)
            pu.prefill_heavy_hitter(cl, layer, k, q, v)
            assert layer.evictions == 0 and layer.rows() == (24, 0) and layer._kalt is None and layer._plan is None
            log = _drive(layer, cl, g, [1] * 20)
            assert [e for _, _, e in log] == ([False] * 7 + [True]) * 2 + [False] * 4
            assert layer.evictions == 2 and layer.get_seq_length() == 70 and layer.stored_length() == 28
        cache.reset()
        assert all(x.get_seq_length() == 0 and x._kbuf is None and x._sbuf is None and x._stail is None and x._kalt is None
                   for x in cache.layers)
