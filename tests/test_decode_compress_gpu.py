"""Decode-stage compression on the MI355X: kvc_decode_compress byte for byte against kvc_compress on the materialised
cat(prefix, repeat_kv(tail)) (and against the CPU oracle on a small case), no host synchronisation on the SPLIT decode path,
and DecodeCompressedCache end to end on a tiny Llama (bounded storage, every compression = the rule, flat memory, SPLIT and
EXPANDED forms identical)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def _bits(t):
    return t.contiguous().view(BITS[t.dtype])


def _state(seed, dtype, b, hkv, G, P, T, W, D, dev, ties=False):
    """Prefix [b, Hq, P(+spare), D], tail [b, Hkv, T(+spare), D] in buffers with spare rows, and a [b, Hq, W, D] query ring."""
    g = torch.Generator().manual_seed(seed)
    hq = hkv * G
    kp = torch.randn(b, hq, P + 5, D, generator=g) * 2
    vp = torch.randn(b, hq, P + 5, D, generator=g)
    kt = torch.randn(b, hkv, T + 7, D, generator=g) * 2
    vt = torch.randn(b, hkv, T + 7, D, generator=g)
    if ties:                                          # repeated keys: many equal scores at the top-k threshold
        kp[:, :, 1::2] = kp[:, :, 0:1]
        kt[:, :, :T - W:3] = kp[:, :1, 0:1].expand(b, hkv, -1, D)[:, :, :1]
    ring = torch.randn(b, hq, W, D, generator=g)
    return [x.to(dtype).to(dev) for x in (kp, vp, kt, vt, ring)]


def _materialise(kp, vp, kt, vt, P, T, G):
    k = torch.cat([kp[:, :, :P], kt[:, :, :T].repeat_interleave(G, 1)], 2)
    v = torch.cat([vp[:, :, :P], vt[:, :, :T].repeat_interleave(G, 1)], 2)
    return k, v


def _window_q(ring, ring_start, L):
    """Full-length queries whose last W rows are the ring's rows in chronological order (the rest is never read)."""
    b, h, W, D = ring.shape
    q = torch.zeros(b, h, L, D, dtype=ring.dtype, device=ring.device)
    q[:, :, L - W:] = torch.roll(ring, -ring_start, dims=2)
    return q


# method, dtype, D, W, G, P, T, bsz, ring_start, tie, kernel, pooling, k, ties
CASES = [
    ("snapkv", torch.bfloat16, 128, 8, 4, 203, 45, 1, 3, "torch_cpu", 7, "maxpool", 60, False),
    ("snapkv", torch.bfloat16, 128, 8, 4, 203, 45, 1, 3, "canonical", 7, "maxpool", 60, False),
    ("snapkv", torch.float16, 128, 16, 8, 150, 171, 2, 5, "torch_cpu", 5, "avgpool", 90, False),
    ("snapkv", torch.float32, 128, 32, 1, 97, 77, 2, 31, "canonical", 7, "avgpool", 40, False),
    ("snapkv", torch.bfloat16, 64, 64, 4, 301, 64, 1, 10, "torch_cpu", 7, "maxpool", 100, False),
    ("snapkv", torch.float32, 64, 12, 8, 61, 139, 2, 7, "torch_cpu", 3, "maxpool", 33, False),
    ("snapkv", torch.float16, 64, 8, 1, 44, 8, 2, 1, "canonical", 1, "avgpool", 20, False),
    ("snapkv", torch.bfloat16, 128, 32, 4, 129, 200, 1, 0, "torch_cpu", 7, "maxpool", 1, False),
    ("snapkv", torch.bfloat16, 128, 16, 4, 230, 33, 2, 9, "torch_cpu", 5, "maxpool", 120, True),
    ("snapkv", torch.float16, 128, 16, 4, 230, 33, 2, 9, "canonical", 5, "avgpool", 120, True),
    ("snapkv", torch.bfloat16, 128, 8, 8, 100, 21, 1, 2, "torch_cpu", 7, "maxpool", 0, False),
    ("pyramidkv", torch.bfloat16, 128, 32, 4, 1000, 160, 1, 17, "torch_cpu", 7, "avgpool", 700, False),
    ("pyramidkv", torch.float32, 128, 8, 4, 77, 300, 2, 6, "canonical", 7, "maxpool", 50, False),
    ("pyramidkv", torch.float16, 64, 64, 1, 130, 70, 2, 63, "torch_cpu", 7, "avgpool", 66, True),
    ("streamingllm", torch.bfloat16, 128, 8, 4, 203, 45, 2, 0, "torch_cpu", 7, None, 60, False),
    ("streamingllm", torch.float32, 64, 16, 8, 33, 16, 1, 0, "torch_cpu", 7, None, 30, False),
    ("streamingllm", torch.float16, 128, 12, 1, 5, 200, 2, 0, "torch_cpu", 7, None, 150, False),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{str(c[1])[6:]}-D{c[2]}-W{c[3]}-G{c[4]}-P{c[5]}-T{c[6]}-b{c[7]}-{c[9]}"
                                            f"{'-ties' if c[13] else ''}-k{c[12]}" for c in CASES])
def test_decode_compress_equals_compress_on_materialised_cache(kvc, gpu_device, case):
    method, dtype, D, W, G, P, T, b, rs, tie, ks, pool, k, ties = case
    mid = {"snapkv": kvc.SNAPKV, "pyramidkv": kvc.PYRAMIDKV, "streamingllm": kvc.STREAMINGLLM}[method]
    hkv = 2
    kp, vp, kt, vt, ring = _state(CASES.index(case), dtype, b, hkv, G, P, T, W, D, gpu_device, ties)
    hq, L = hkv * G, P + T
    kb = torch.full((b, hq, k + W + 3, D), float("nan"), dtype=dtype, device=gpu_device)
    vb = torch.full_like(kb, float("nan"))
    scoring = method != "streamingllm"
    res = kvc.decode_compress(mid, ring, rs, kp, vp, P, kt, vt, T, (kb, vb), W, k, ks, pool if scoring else None, tie,
                              return_indices=True, return_scores=scoring)
    K, V = _materialise(kp, vp, kt, vt, P, T, G)
    q = _window_q(ring, rs, L) if scoring else None
    ref = kvc.compress(mid, q, K, V, W, k, ks, pool if scoring else None, tie, n_q_heads=hq, return_indices=True,
                       return_scores=scoring, dot_mode="exact")
    torch.cuda.synchronize()
    assert torch.equal(_bits(res[0]), _bits(ref[0])) and torch.equal(_bits(res[1]), _bits(ref[1]))
    assert torch.equal(res[2], ref[2])
    if scoring:
        assert torch.equal(_bits(res[3]), _bits(ref[3]))
    assert torch.isnan(kb[:, :, k + W:].float()).all()                        # nothing written past the kept rows


def test_decode_compress_small_case_against_cpu_oracle(kvc, oracle, gpu_device):
    O = oracle
    dtype, D, W, G, P, T, k, rs = torch.bfloat16, 128, 8, 4, 90, 37, 40, 5
    kp, vp, kt, vt, ring = _state(7, dtype, 1, 2, G, P, T, W, D, gpu_device)
    kb = torch.empty(1, 2 * G, k + W, D, dtype=dtype, device=gpu_device)
    vb = torch.empty_like(kb)
    ko, vo, idx, sc = kvc.decode_compress(kvc.SNAPKV, ring, rs, kp, vp, P, kt, vt, T, (kb, vb), W, k, 7, "maxpool", "torch_cpu",
                                          return_indices=True, return_scores=True)
    K, V = _materialise(kp, vp, kt, vt, P, T, G)
    q = _window_q(ring, rs, P + T)
    ko_o, vo_o, idx_o, sc_o = O.compress(q.cpu(), K.cpu().contiguous(), V.cpu().contiguous(), W, k, 7, "maxpool", dot_mode=O.DOT_CHAIN,
                                         sum_mode=O.SUM_TORCH16, tie_mode=O.TIES_TORCH)
    assert torch.equal(_bits(sc[0].cpu()), _bits(sc_o))
    assert torch.equal(idx[0].cpu(), idx_o)
    assert torch.equal(_bits(ko.cpu()), _bits(ko_o)) and torch.equal(_bits(vo.cpu()), _bits(vo_o))


# ---- the layer ---------------------------------------------------------------------------------------------------------------
def _prefilled_layer(dev, P0=40, hq=8, D=128, interval=16, seed=0):
    from kvcache_factory_amd.cache import DecodeCompressedLayer
    g = torch.Generator().manual_seed(seed)
    layer = DecodeCompressedLayer(interval)
    kc = (torch.randn(1, hq, P0, D, generator=g)).to(torch.bfloat16).to(dev)
    vc = (torch.randn(1, hq, P0, D, generator=g)).to(torch.bfloat16).to(dev)
    layer.prefill(kc, vc, 500)
    return layer, g


def _rows(g, dev, n, hq=8, hkv=2, D=128, t=1):
    """n steps' (q, k, v), made on the device up front (a copy from pageable host memory synchronises)."""
    mk = lambda h: torch.randn(1, h, t, D, generator=g).to(torch.bfloat16).to(dev)
    return [(mk(hq), mk(hkv), mk(hkv)) for _ in range(n)]


def test_split_decode_path_has_no_host_synchronisation(kvc, gpu_device):
    """A few SPLIT decode steps with one compression under sync debug mode "error": kvc_decode_step2 (decode_attend), the ring
    writes and kvc_decode_compress."""
    from kvcache_factory_amd import pyramidkv_utils as pu
    cl = pu.SnapKVCluster(window_size=8, max_capacity_prompt=40, kernel_size=7, pooling="maxpool")
    layer, g = _prefilled_layer(gpu_device)
    warm, steps = _rows(g, gpu_device, 3), _rows(g, gpu_device, 16)
    for q, k, v in warm:                                    # the tail exists, the decode step's workspace too
        layer.decode_attend(q, k, v, 128 ** -0.5)
        layer.after_decode(cl, q)
    torch.cuda.synchronize()
    n0 = layer.compressions
    torch.cuda.set_sync_debug_mode("error")
    try:
        for q, k, v in steps:
            layer.decode_attend(q, k, v, 128 ** -0.5)
            layer.after_decode(cl, q)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert layer.compressions == n0 + 1 and layer.stored_length() <= 40 + 16


@pytest.mark.parametrize("dot_mode", ["exact", "mfma16"])
def test_split_and_expanded_forms_compress_to_identical_bytes(kvc, gpu_device, dot_mode, monkeypatch):
    """The same steps through the SPLIT form (decode_attend) and the EXPANDED form (update with repeat_kv rows): every
    compression leaves identical bytes, also when KVC_DOT_MODE says mfma16 (which does not apply at decode time)."""
    from kvcache_factory_amd import pyramidkv_utils as pu
    monkeypatch.setattr(kvc, "DOT_MODE", dot_mode)
    for method, cl in (("snapkv", pu.SnapKVCluster(window_size=8, max_capacity_prompt=40, kernel_size=7, pooling="maxpool")),
                       ("pyramidkv", pu.PyramidKVCluster(num_hidden_layers=4, window_size=8, max_capacity_prompt=40, layer_idx=1)),
                       ("streamingllm", pu.StreamingLLMKVCluster(window_size=8, max_capacity_prompt=40))):
        a, g = _prefilled_layer(gpu_device, interval=16, seed=1)
        b, _ = _prefilled_layer(gpu_device, interval=16, seed=1)
        for i in range(50):
            t = 3 if i % 7 == 0 else 1
            q = torch.randn(1, 8, t, 128, generator=g).to(torch.bfloat16).to(gpu_device)
            k = torch.randn(1, 2, t, 128, generator=g).to(torch.bfloat16).to(gpu_device)
            v = torch.randn(1, 2, t, 128, generator=g).to(torch.bfloat16).to(gpu_device)
            a.decode_attend(q, k, v, 128 ** -0.5)
            a.after_decode(cl, q)
            b.update(k.repeat_interleave(4, 1), v.repeat_interleave(4, 1))
            b.after_decode(cl, q)
            assert a.stored_length() == b.stored_length()
        torch.cuda.synchronize()
        assert a._split and not b._split
        assert a.compressions == b.compressions >= 2, method
        assert torch.equal(_bits(a.keys), _bits(b.keys)) and torch.equal(_bits(a.values), _bits(b.values)), method


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["snapkv", "pyramidkv", "streamingllm"])
def test_generate_with_decode_compression(kvc, gpu_device, method, monkeypatch):
    from transformers import LlamaConfig, LlamaForCausalLM
    from kvcache_factory_amd import DecodeCompressedCache, monkeypatch as mp, pyramidkv_utils as pu
    from kvcache_factory_amd.cache import DecodeCompressedLayer
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=256, num_hidden_layers=3, num_attention_heads=32,
                      num_key_value_heads=8, head_dim=128, vocab_size=256, max_position_embeddings=4096, attn_implementation="sdpa")
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).to(gpu_device).eval()
    L, cap, W, interval, new = 300, 64, 8, 32, 240
    ids = torch.randint(0, 256, (1, L), generator=torch.Generator().manual_seed(3)).to(gpu_device)
    mid = {"snapkv": kvc.SNAPKV, "pyramidkv": kvc.PYRAMIDKV, "streamingllm": kvc.STREAMINGLLM}[method]
    history = {}                      # layer -> post-RoPE queries of every decoded row
    checked = {}                      # layer -> compressions checked against the rule
    mems = []                         # memory_allocated after every step once each layer has compressed twice
    peak = {}
    orig_after, orig_compress = DecodeCompressedLayer.after_decode, DecodeCompressedLayer._compress

    def after(self, cluster, q):
        i = id(self)
        history.setdefault(i, []).append(q.detach().cpu())        # kept off the device: memory_allocated is checked
        P, T = self.rows()
        if self.compressions:
            peak[i] = max(peak.get(i, 0), P + T - (q.shape[-2] - 1))
        return orig_after(self, cluster, q)

    def compress(self, cluster, m, B, W_, P, T):
        K, V = self.keys.clone(), self.values.clone()
        S = P + T
        qs = torch.cat(history[id(self)], 2)[:, :, -W_:].to(K.device)
        if m != kvc.STREAMINGLLM:
            assert torch.equal(_bits(torch.roll(self._qring, -(S % W_), dims=2)), _bits(qs))      # ring in chronological order
        orig_compress(self, cluster, m, B, W_, P, T)
        q = torch.zeros(K.shape[0], K.shape[1], S, K.shape[3], dtype=K.dtype, device=K.device)
        q[:, :, S - W_:] = qs
        ko, vo = kvc.compress(m, q if m != kvc.STREAMINGLLM else None, K, V, W_, B - W_, cluster.kernel_size,
                              cluster.pooling if m != kvc.STREAMINGLLM else None, pu.TIE_MODE, n_q_heads=K.shape[1], dot_mode="exact")
        assert self.stored_length() == B and self.keys.shape[2] == B
        assert torch.equal(_bits(self.keys), _bits(ko)) and torch.equal(_bits(self.values), _bits(vo))
        checked[id(self)] = checked.get(id(self), 0) + 1

    monkeypatch.setattr(DecodeCompressedLayer, "after_decode", after)
    monkeypatch.setattr(DecodeCompressedLayer, "_compress", compress)
    try:
        mp.replace_llama(method)
        for layer in model.model.layers:
            for name, val in (("window_size", W), ("max_capacity_prompt", cap), ("kernel_size", 7), ("pooling", "maxpool")):
                setattr(layer.self_attn.config, name, val)
        cache = DecodeCompressedCache(model.config, interval=interval)
        with torch.no_grad():                  # greedy decoding by hand: generate()'s growing token tensors would hide a flat cache
            logits = model(ids, past_key_values=cache, use_cache=True).logits
            for _ in range(new - 1):
                logits = model(logits[:, -1:].argmax(-1), past_key_values=cache, use_cache=True).logits
                if all(x.compressions >= 2 for x in cache.layers):     # after the second compression cycle of every layer
                    torch.cuda.synchronize()
                    mems.append(torch.cuda.memory_allocated())
    finally:
        mp.replace_llama("fullkv")
    for li, layer in enumerate(cache.layers):
        _, B, _ = layer._plan
        if method == "pyramidkv":
            cl = pu.PyramidKVCluster(num_hidden_layers=3, window_size=W, max_capacity_prompt=cap, layer_idx=li)
            assert B == kvc.pyramid_k(cap, W, 2 * cap, li, 3) + W == cl._budget(2 * cap) + W
        else:
            assert B == cap
        i = id(layer)
        assert checked.get(i, 0) >= 3 and checked[i] == layer.compressions, (li, checked.get(i), layer.compressions)
        assert peak[i] <= B + interval, (li, peak[i], B)
        assert layer.get_seq_length() == L + new - 1
        assert layer.get_mask_sizes(1)[0] == layer.stored_length() + 1 <= B + interval
        assert layer._kbuf.shape[2] == B and layer._kalt.shape[2] == B          # two prefix buffers of exactly B rows
    assert len(mems) >= 2 * interval and len(set(mems)) == 1, sorted(set(mems))
