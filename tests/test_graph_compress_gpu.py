"""Decode-stage compression under graph-replayed decoding on the MI355X.

The entry (kvc_decode_step_dev_ring): the conformance harness of tests/decode_ref.py through an adapter that adds a NaN-filled query
ring to test_graph_decode_gpu's NaN-filled tail (needles bit for bit, the per-element bound at the harness's factor, ring slot
(T + i) % W = query row i for i >= t - W and every other slot untouched), and the ring's edges in direct calls whose outputs equal
kvc_decode_step_dev's bit for bit.  The layer (cache.BoundedDeviceLayer) beside the host-counted DecodeCompressedLayer on the same rows.
End to end: GraphDecoder(model, interval=N) replayed against capture=False, one capture, no growth, the ring and every compression
against the rule on the materialised rows, flat memory, no host synchronisation."""
import numpy as np
import pytest
import torch

import decode_ref as R
from test_decode_conformance_cpu import run_bound, run_needles
from test_graph_decode_cpu import dev_split_plan

pytestmark = pytest.mark.gpu

BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(BITS[t.dtype])


def _ring_after(q, T, W):
    """What a NaN-filled ring [b, H_q, W, D] holds after a step of q's rows that read the (clamped) counter value T."""
    ring = torch.full((q.shape[0], q.shape[1], W, q.shape[3]), NAN, dtype=q.dtype, device=q.device)
    t = q.shape[2]
    for i in range(max(0, t - W), t):
        ring[:, :, (T + i) % W] = q[:, :, i]
    return ring


# ---- 1. conformance through the existing harness ------------------------------------------------------------------------------------
W_CONF = 8
SPECS = [s for s in R.GRID if s["entry"] == "step2" and not s.get("P1")]
CAPS = {"own": lambda T, t: T + t, "wide": lambda T, t: T + t + 1024}
CONF = [(s, c) for s in SPECS for c in CAPS]
CONF_IDS = [f"{R.spec_id(s)}-{c}" for s, c in CONF]


def adapter(kvc, capacity_of, seen=None):
    """decode_step's signature over kvc_decode_step_dev_ring: test_graph_decode_gpu.adapter plus a NaN-filled ring of W_CONF slots."""
    def run(q, kn, vn, kp, vp, P, kt, vt, T, scaling):
        b, hkv, _, D = kt.shape
        t = q.shape[2]
        cap = capacity_of(T, t)
        bk = torch.full((b, hkv, cap, D), NAN, dtype=kt.dtype, device=kt.device)
        bv = torch.full_like(bk, NAN)
        bk[:, :, :T], bv[:, :, :T] = kt[:, :, :T], vt[:, :, :T]
        counter = torch.tensor([T], dtype=torch.int32, device=kt.device)
        ring = torch.full((b, q.shape[1], W_CONF, D), NAN, dtype=q.dtype, device=q.device)
        out = kvc.decode_step_dev_ring(q, kn, vn, kp, vp, P, bk, bv, counter, scaling, ring)
        kt[:, :, :T + t], vt[:, :, :T + t] = bk[:, :, :T + t], bv[:, :, :T + t]
        assert torch.isnan(bk[:, :, T + t:].float()).all() and torch.isnan(bv[:, :, T + t:].float()).all()
        assert int(counter) == T                                             # the library only reads it
        assert torch.equal(_bits(ring), _bits(_ring_after(q, T, W_CONF))), "ring slots"
        if seen is not None:
            seen.append(dev_split_plan(b, q.shape[1], t, P, cap)[0])
        return out
    return run


@pytest.mark.parametrize("spec,cap", CONF, ids=CONF_IDS)
def test_conformance_needles_row_exact(kvc, gpu_device, spec, cap):
    seen = []
    probes = run_needles(spec, adapter(kvc, CAPS[cap], seen), gpu_device)
    assert cap == "own" or min(seen) > 1                                     # the wide bound really ran split
    print(f"{R.spec_id(spec)} ({cap}, {max(seen)} splits): {probes} needles returned their row")


@pytest.mark.parametrize("spec,cap", CONF, ids=CONF_IDS)
def test_conformance_per_element_bound(kvc, gpu_device, spec, cap):
    e_kernel, e_ref = run_bound(spec, adapter(kvc, CAPS[cap]), gpu_device)
    print(f"{R.spec_id(spec)} ({cap}): e_kernel / e_ref = {e_kernel / e_ref:.3f} (e_ref = {e_ref:.3e})")
    assert e_kernel <= R.FACTOR * e_ref


# ---- 2. the ring's edges, direct calls ---------------------------------------------------------------------------------------------
HQ, HKV, P0, CAP = 8, 2, 40, 24


@pytest.mark.parametrize("W", [1, 8, 32])
@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.bfloat16, 64), (torch.float32, 128), (torch.float32, 64)])
def test_ring_edges(kvc, gpu_device, dtype, D, W):
    """t in {1, 3, W + 2} x counter values {0, W - 1, W, capacity - t} at capacity 24 (a value past capacity - t is clamped, and the
    ring follows the clamped one).  A step of more rows than the tail holds cannot run: skipped and counted — none for W <= 8."""
    g = torch.Generator().manual_seed(W * 1000 + D)
    mk = lambda *sh: torch.randn(*sh, generator=g).to(dtype).to(gpu_device)  # noqa: E731
    kp, vp, live_k, live_v = mk(1, HQ, P0, D), mk(1, HQ, P0, D), mk(1, HKV, CAP, D), mk(1, HKV, CAP, D)
    skipped = ran = 0
    for t in (1, 3, W + 2):
        if t > CAP:
            skipped += 4
            continue
        q, kn, vn = mk(1, HQ, t, D), mk(1, HKV, t, D), mk(1, HKV, t, D)
        for value in (0, W - 1, W, CAP - t):
            T = min(max(value, 0), CAP - t)
            res = []
            for entry in ("ring", "plain"):
                kt, vt = torch.full((1, HKV, CAP, D), NAN, dtype=dtype, device=gpu_device), torch.full((1, HKV, CAP, D), NAN, dtype=dtype,
                                                                                                   device=gpu_device)
                kt[:, :, :T], vt[:, :, :T] = live_k[:, :, :T], live_v[:, :, :T]
                counter = torch.tensor([value], dtype=torch.int32, device=gpu_device)
                n = kvc.decode_dev_plan(q, kn, kp, P0, kt)[1]
                ws = torch.empty(max(n, 16), dtype=torch.uint8, device=gpu_device)
                if entry == "ring":
                    ring = torch.full((1, HQ, W, D), NAN, dtype=dtype, device=gpu_device)
                    out = kvc.decode_step_dev_ring(q, kn, vn, kp, vp, P0, kt, vt, counter, D ** -0.5, ring, ws=ws)
                    assert torch.equal(_bits(ring), _bits(_ring_after(q, T, W))), (t, value)
                else:
                    out = kvc.decode_step_dev(q, kn, vn, kp, vp, P0, kt, vt, counter, D ** -0.5, ws=ws)
                assert int(counter) == value
                res.append((out, kt, vt))
            for x, y in zip(*res):
                assert torch.equal(_bits(x), _bits(y)), (t, value)
            assert torch.isfinite(res[0][0].float()).all()
            assert torch.equal(_bits(res[0][1][:, :, T:T + t]), _bits(kn)) and torch.isnan(res[0][1][:, :, T + t:].float()).all()
            ran += 1
    assert ran + skipped == 12 and (skipped == 0 if W <= 8 else skipped == 4)


# ---- 3. the layer beside the host-counted one -----------------------------------------------------------------------------------------
def _cluster(method, W=8, cap=40):
    from kvcache_factory_amd import pyramidkv_utils as pu
    if method == "snapkv":
        return pu.SnapKVCluster(window_size=W, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool")
    if method == "pyramidkv":
        return pu.PyramidKVCluster(num_hidden_layers=4, window_size=W, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool", layer_idx=1)
    return pu.StreamingLLMKVCluster(window_size=W, max_capacity_prompt=cap)


def _check_step_bound(out, q, K, V, scaling):
    """decode_ref's per-element bound for one token over the materialised rows K / V [1, H_q, n, D] (the step's own row last)."""
    dtype = q.dtype
    q64, K64, V64 = R._np64(q), R._np64(K), R._np64(V)
    n = np.full((1, q.shape[1]), K.shape[2])
    ref, p = R.attention64(q64, K64, V64, n, scaling)
    pv = np.einsum("bhtr,bhrd->bhtd", p, np.abs(V64))
    w = torch.softmax(torch.einsum("bhtd,bhrd->bhtr", q.float().cpu(), K.float().cpu()) * scaling, -1)
    ref32 = R._np64(torch.einsum("bhtr,bhrd->bhtd", w, V.float().cpu()).to(dtype))
    e_ref = float((np.abs(ref32 - ref) / pv).max())
    got = R._np64(out.transpose(1, 2))                                       # [1, t, H_q, D] -> [1, H_q, t, D]
    err = np.abs(got - ref)
    half = 0.5 * R.ulp(np.maximum(np.abs(ref), np.abs(got)), dtype)
    assert np.isfinite(got).all() and not (err > half + R.FACTOR * e_ref * pv).any()


@pytest.mark.parametrize("P0_", [20, 40, 45])
@pytest.mark.parametrize("method", ["snapkv", "pyramidkv", "streamingllm"])
def test_bounded_layer_beside_the_host_counted_layer(kvc, gpu_device, method, P0_):
    """hq 8, hkv 2, D 128, bf16, W 8, max_capacity_prompt 40, interval 16, one-token steps with a real device counter.  50 steps, or
    as many as the second compression needs: from P0 = 20 the first comes after B + 16 - 20 steps and the second 16 later, which is
    step 52 at B = 40 — 50 steps would hold one compression there."""
    from kvcache_factory_amd.cache import BoundedDeviceLayer, CompressedDynamicLayer, DecodeCompressedLayer, decode_budget
    hq, hkv, D, interval = 8, 2, 128, 16
    cl = _cluster(method)
    _, B, W = decode_budget(cl, interval)
    steps = max(50, max(W, B + interval - P0_) + interval)
    g = torch.Generator().manual_seed(P0_)
    mk = lambda *sh: torch.randn(*sh, generator=g).to(torch.bfloat16).to(gpu_device)  # noqa: E731
    k0, v0 = mk(1, hq, P0_, D), mk(1, hq, P0_, D)
    host, plain = DecodeCompressedLayer(interval), CompressedDynamicLayer()
    host.prefill(k0.clone(), v0.clone(), 500)
    plain.prefill(k0.clone(), v0.clone(), 500)
    counters = torch.full((3,), 77, dtype=torch.int32, device=gpu_device)
    layer = BoundedDeviceLayer.adopt(plain, cl, interval, counters[1:2], hkv)
    at = []
    for step in range(steps):
        q, k, v = mk(1, hq, 1, D), mk(1, hkv, 1, D), mk(1, hkv, 1, D)
        K = torch.cat([layer.keys, k.repeat_interleave(hq // hkv, 1)], 2)
        V = torch.cat([layer.values, v.repeat_interleave(hq // hkv, 1)], 2)
        n0 = host.compressions
        ref = host.decode_attend(q, k, v, D ** -0.5)
        host.after_decode(cl, q)
        out = layer.decode_attend(q, k, v, D ** -0.5)
        _check_step_bound(out, q, K, V, D ** -0.5)
        _check_step_bound(ref, q, K, V, D ** -0.5)
        counters[1:2].add_(1)
        layer.advance(1)
        did = layer.maybe_compress()
        assert did == (host.compressions > n0), step
        assert layer.stored_length() == host.stored_length() and layer.rows() == host.rows(), step
        assert int(layer._plen) == layer._stored and counters.tolist() == [77, layer._tail, 77]
        if did:
            at.append(step)
            assert layer.stored_length() == B
            assert torch.equal(_bits(layer.keys), _bits(host.keys)) and torch.equal(_bits(layer.values), _bits(host.values)), step
    assert len(at) >= 2 and layer.compressions == host.compressions == len(at)
    assert torch.equal(_bits(layer.keys), _bits(host.keys)) and torch.equal(_bits(layer.values), _bits(host.values))


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------
class _Model:
    """The 3-layer model of test_generate_with_decode_compression with the forwards of `method` patched in (restored on exit)."""

    def __init__(self, method, cap=64, window=8):
        self.method, self.cap, self.window = method, cap, window

    def __enter__(self):
        from transformers import LlamaConfig, LlamaForCausalLM
        from kvcache_factory_amd import monkeypatch as mp
        mp.replace_llama(self.method)
        torch.manual_seed(0)
        cfg = LlamaConfig(hidden_size=4096, intermediate_size=256, num_hidden_layers=3, num_attention_heads=32, num_key_value_heads=8,
                          head_dim=128, vocab_size=256, max_position_embeddings=4096, attn_implementation="sdpa")
        model = LlamaForCausalLM(cfg).to(torch.bfloat16).to("cuda:0").eval()
        for layer in model.model.layers:
            for name, val in (("window_size", self.window), ("max_capacity_prompt", self.cap), ("kernel_size", 7), ("pooling", "maxpool")):
                setattr(layer.self_attn.config, name, val)
        return model

    def __exit__(self, *exc):
        from kvcache_factory_amd import monkeypatch as mp
        mp.replace_llama("fullkv")


@pytest.mark.parametrize("method", ["snapkv", "pyramidkv", "streamingllm"])
def test_replayed_generation_with_decode_compression(kvc, gpu_device, method, monkeypatch):
    """L 300, cap 64, W 8, interval 32, 240 new tokens, the replayed decoder and capture=False in lockstep; then 40 more replayed
    steps (one compression per layer among them) under sync debug mode "error"."""
    from kvcache_factory_amd import GraphDecoder, pyramidkv_utils as pu
    from kvcache_factory_amd.cache import BoundedDeviceLayer, decode_trigger
    L, cap, W, interval, new = 300, 64, 8, 32, 240
    ids = torch.randint(0, 256, (1, L), generator=torch.Generator().manual_seed(3)).to(gpu_device)
    who = {}                          # id(layer) -> layer index (both decoders)
    history = {}                      # layer index -> post-RoPE queries of every decoded row, from the eager decoder's Python
    checked = {}                      # id(layer) -> compressions checked against the rule
    checking = [True]
    orig_attend, orig_compress = BoundedDeviceLayer._decode_attend_dev, BoundedDeviceLayer.maybe_compress

    def attend(self, q, k, v, scaling):
        if checking[0] and self in eager._layers:
            history.setdefault(who[id(self)], []).append(q.detach().cpu())
        return orig_attend(self, q, k, v, scaling)

    def compress(self):
        m, B, W_ = self._plan
        P, T = self.rows()
        if not checking[0] or not decode_trigger(P, T, B, W_, self.interval):
            return orig_compress(self)
        K, V = self.keys.clone(), self.values.clone()
        n0 = self.compressions
        did = orig_compress(self)
        if did:
            S = P + T
            qs = torch.cat(history[who[id(self)]], 2)[:, :, -W_:].to(K.device)          # the last W recorded queries
            assert len(history[who[id(self)]]) == self.get_seq_length() - L and T >= W_
            if m != kvc.STREAMINGLLM:
                assert torch.equal(_bits(torch.roll(self._qring, -(T % W_), dims=2)), _bits(qs))   # the ring in chronological order
            q = torch.zeros(1, K.shape[1], S, K.shape[3], dtype=K.dtype, device=K.device)
            q[:, :, S - W_:] = qs
            cl = self._cluster
            ko, vo = kvc.compress(m, q if m != kvc.STREAMINGLLM else None, K, V, W_, B - W_, cl.kernel_size,
                                  cl.pooling if m != kvc.STREAMINGLLM else None, pu.TIE_MODE, n_q_heads=K.shape[1], dot_mode="exact")
            assert self.compressions == n0 + 1 and self.stored_length() == B and self.keys.shape[2] == B
            assert torch.equal(_bits(self.keys), _bits(ko)) and torch.equal(_bits(self.values), _bits(vo))
            checked[id(self)] = checked.get(id(self), 0) + 1
        return did

    monkeypatch.setattr(BoundedDeviceLayer, "_decode_attend_dev", attend)
    monkeypatch.setattr(BoundedDeviceLayer, "maybe_compress", compress)
    with _Model(method, cap, W) as model:
        replay, eager = GraphDecoder(model, interval=interval), GraphDecoder(model, interval=interval, capture=False)
        le, lr = eager.prefill(ids).clone(), replay.prefill(ids).clone()
        assert torch.equal(_bits(le), _bits(lr))
        for dec in (replay, eager):
            assert all(type(x) is BoundedDeviceLayer for x in dec._cache.layers)
            who.update({id(x): i for i, x in enumerate(dec._layers)})
        budgets = [x._plan[1] for x in replay._layers]
        if method == "pyramidkv":
            assert budgets == [kvc.pyramid_k(cap, W, 2 * cap, li, 3) + W for li in range(3)]
        else:
            assert budgets == [cap] * 3
        tok = torch.empty(1, 1, dtype=torch.long, device=gpu_device)
        mems = []
        for j in range(new - 1):
            tok.copy_(le[:, -1].argmax(-1, keepdim=True))
            le = eager.step(tok)                                             # (the static buffers: compared before the next step)
            lr = replay.step(tok)
            assert torch.equal(_bits(le), _bits(lr)), f"step {j}"
            if all(x.compressions >= 1 for x in replay._layers + eager._layers):
                torch.cuda.synchronize()
                mems.append(torch.cuda.memory_allocated())
        assert replay.captures == 1 and replay.grows == 0 and eager.captures == 0 and eager.grows == 0
        for dec in (replay, eager):
            for li, layer in enumerate(dec._layers):
                assert checked.get(id(layer), 0) >= 3 and checked[id(layer)] == layer.compressions, (li, checked.get(id(layer)))
                assert layer.get_seq_length() == L + new - 1 and layer.stored_length() <= budgets[li] + interval
                assert int(layer._plen) == layer._stored and int(layer._dev_counter) == layer._tail
        for a, b in zip(replay._layers, eager._layers):
            assert a.rows() == b.rows()
            assert torch.equal(_bits(a.keys), _bits(b.keys)) and torch.equal(_bits(a.values), _bits(b.values))
        assert len(mems) >= 2 * interval and len(set(mems)) == 1, sorted(set(mems))
        assert replay._cache.get_seq_length() == L + new - 1 and replay._pos.tolist() == [[L + new - 1]]
        # replays and a compression of every layer without a host synchronisation, memory still flat
        checking[0] = False
        n0 = [x.compressions for x in replay._layers]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(interval + W):
                replay.step(tok)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        assert all(x.compressions > n for x, n in zip(replay._layers, n0))
        assert torch.cuda.memory_allocated() == mems[-1] and replay.captures == 1 and replay.grows == 0
