"""The heavy-hitter cache on the GPU: kvc_decode_step_scored against kvc_decode_step2 (attention bytes) and against an fp64
restatement of the scoring rule (one-step bound from the fp32 torch restatement's own error), determinism and bounds,
kvc_decode_evict against torch.topk and a torch gather (exact), a chain of evictions, H2O's behaviour on a synthetic layer, and
greedy generation with tiny random Llama / Mistral models past three evictions of every layer."""
import pytest
import torch

import heavy_hitter_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
LENGTHS = [(40, 10), (500, 201)]          # (prefix rows, tail rows): one split, several


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _case(dev, dtype, D, G, t, P, T, seed=0, spare=5):
    """A layer's state before a step of t tokens: unit-variance K, queries of standard deviation 1.5.  Buffers hold `spare` rows
    more than the step makes visible."""
    g = torch.Generator().manual_seed(seed)
    hq, hkv = 8, 8 // G
    mk = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dtype).to(dev)
    c = dict(q=mk(1, hq, t, D, s=1.5), k_new=mk(1, hkv, t, D), v_new=mk(1, hkv, t, D), kp=mk(1, hq, P + spare, D), vp=mk(1, hq, P + spare, D),
             kt=mk(1, hkv, T + t + spare, D), vt=mk(1, hkv, T + t + spare, D), P=P, T=T, t=t, G=G, scaling=D ** -0.5)
    c["sp"] = torch.zeros(1, hq, P + spare, dtype=torch.float32, device=dev)
    c["st"] = torch.zeros(1, hq, T + t + spare, dtype=torch.float32, device=dev)
    return c


def _scored(kvc, c, ws=None):
    return kvc.decode_step_scored(c["q"], c["k_new"], c["v_new"], c["kp"], c["vp"], c["P"], c["kt"], c["vt"], c["T"], c["sp"], c["st"],
                                  c["scaling"], ws=ws)


def _clone(c):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in c.items()}


GRID = [(dt, D, G, t, PT) for dt in DTYPES for D in (64, 128) for G in (1, 4) for t in (1, 3) for PT in LENGTHS]
IDS = [f"{str(dt)[6:]}-D{D}-G{G}-t{t}-P{PT[0]}T{PT[1]}" for dt, D, G, t, PT in GRID]


@pytest.mark.parametrize("dtype,D,G,t,PT", GRID, ids=IDS)
def test_scored_step(kvc, gpu_device, dtype, D, G, t, PT):
    """Attention unchanged (the bytes of kvc_decode_step2), the scores of one step against fp64 (kernel error <= 4 x the fp32 torch
    restatement's on the same tensors, every row compared), determinism, and nothing at or past the visible rows read or written."""
    P, T = PT
    c = _case(gpu_device, dtype, D, G, t, P, T, seed=P + D + G + t)
    a, b = _clone(c), _clone(c)
    ref = kvc.decode_step(a["q"], a["k_new"], a["v_new"], a["kp"], a["vp"], P, a["kt"], a["vt"], T, a["scaling"])
    out = _scored(kvc, b)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(ref))
    assert torch.equal(_bits(a["kt"][:, :, :T + t]), _bits(b["kt"][:, :, :T + t])) and torch.equal(_bits(a["vt"][:, :, :T + t]), _bits(b["vt"][:, :, :T + t]))
    # scores from zero: the increment itself
    p64, e_ref = R.one_step_bound(b["q"], b["kp"], b["kt"], P, T, b["scaling"])
    rows = P + T + t
    got = torch.cat([b["sp"][:, :, :P], b["st"][:, :, :T + t]], 2)
    e_kernel = R.max_rel_err(got, R.step_increment(p64, rows))
    print(f"one-step max relative error: kernel {e_kernel:.3e}, fp32 torch {e_ref:.3e}")
    assert e_kernel <= 4 * e_ref, (e_kernel, e_ref)
    # from scores of known non-zero content (and junk where the step's own rows will be): rule 2 within the one-step bound
    g = torch.Generator().manual_seed(1)
    d = _clone(c)
    d["sp"][:, :, :P] = (torch.rand(1, 8, P, generator=g) * 10).to(gpu_device)
    d["st"][:, :, :T] = (torch.rand(1, 8, T, generator=g) * 10).to(gpu_device)
    d["st"][:, :, T:T + t] = 123.0
    before = torch.cat([d["sp"][:, :, :P], d["st"][:, :, :T + t]], 2).clone()
    _scored(kvc, d)
    R.check_step(before, torch.cat([d["sp"][:, :, :P], d["st"][:, :, :T + t]], 2), p64, e_ref, P + T)
    # determinism; NaN in the workspace and in every row that is not visible yet: same bytes, those rows untouched
    e = _clone(c)
    nan = float("nan")
    for name, lo in (("kp", P), ("vp", P), ("sp", P), ("kt", T + t), ("vt", T + t), ("st", T)):
        e[name][:, :, lo:] = nan
    ws = torch.full((kvc.lib().kvc_decode_scored_workspace_bytes(_params(kvc, e)) // 4 + 64,), nan, dtype=torch.float32, device=gpu_device)
    out_e = _scored(kvc, e, ws=ws.view(torch.uint8))
    out_b2 = _scored(kvc, _clone(c))
    torch.cuda.synchronize()
    assert torch.equal(_bits(out_e), _bits(out)) and torch.equal(_bits(out_b2), _bits(out))
    for name, hi in (("sp", P), ("st", T + t)):
        assert torch.equal(_bits(e[name][:, :, :hi]), _bits(b[name][:, :, :hi])), name
    for name, lo in (("kp", P), ("vp", P), ("sp", P), ("kt", T + t), ("vt", T + t), ("st", T + t)):
        assert bool(torch.isnan(e[name][:, :, lo:].float()).all()), name


def _params(kvc, c):
    import ctypes
    out = torch.empty(1, c["t"], 8, c["q"].shape[3], dtype=c["q"].dtype, device=c["q"].device)
    return ctypes.byref(kvc.decode_scored_params(c["q"], c["k_new"], c["kp"], c["P"], c["kt"], c["T"], c["sp"], c["st"], out, c["scaling"]))


# ---- eviction ----------------------------------------------------------------------------------------------------------------
def _evict_case(dev, dtype, D, G, P, T, kind, seed=0, spare=3):
    g = torch.Generator().manual_seed(seed)
    hq, hkv = 8, 8 // G
    mk = lambda *sh: torch.randn(*sh, generator=g).to(dtype).to(dev)
    kp, vp, kt, vt = mk(1, hq, P + spare, D), mk(1, hq, P + spare, D), mk(1, hkv, T + spare, D), mk(1, hkv, T + spare, D)
    S = P + T
    if kind == "random":
        sc = torch.rand(1, hq, S, generator=g) * 10
    elif kind == "plateaus":                                          # few distinct values: the threshold falls inside a plateau
        sc = torch.randint(0, 6, (1, hq, S), generator=g).float() * 0.25
    else:
        sc = torch.zeros(1, hq, S)
    sp = torch.full((1, hq, P + spare), float("nan"))
    st = torch.full((1, hq, T + spare), float("nan"))
    sp[:, :, :P], st[:, :, :T] = sc[:, :, :P], sc[:, :, P:]
    return kp, vp, kt, vt, sp.to(dev), st.to(dev)


@pytest.mark.parametrize("tie", ["torch_cpu", "canonical"])
@pytest.mark.parametrize("kind", ["random", "plateaus", "zeros"])
@pytest.mark.parametrize("dtype,D,G", [(torch.bfloat16, 128, 4), (torch.float16, 64, 1), (torch.bfloat16, 64, 4), (torch.float16, 128, 1)])
def test_eviction_is_exact(kvc, gpu_device, dtype, D, G, kind, tie):
    """idx_out = torch.topk on the CPU of exactly the fp32 scores read back (torch_cpu) / value descending, index ascending
    (canonical); K', V' and the kept scores equal the torch gather byte for byte.  Cases on both sides of k * 64 = n."""
    W = 16
    for P, T, k in ((300, 80, 5), (300, 80, 6), (300, 80, 200), (0, 120, 40), (64, 16, 48), (2048, 128, 31), (2048, 128, 2016)):
        kp, vp, kt, vt, sp, st = _evict_case(gpu_device, dtype, D, G, P, T, kind, seed=P + k)
        rows = k + W
        kout = torch.full((1, 8, rows + 2, D), 7.0, dtype=dtype, device=gpu_device)
        vout, sout = kout.clone(), torch.full((1, 8, rows + 2), 7.0, dtype=torch.float32, device=gpu_device)
        ko, vo, so, idx = kvc.decode_evict(kp, vp, P, kt, vt, T, sp, st, (kout, vout), sout, W, k, tie, return_indices=True)
        torch.cuda.synchronize()
        score = torch.cat([sp[:, :, :P], st[:, :, :T]], 2)
        K, V = R.virtual_rows(kp, kt, P, T, G), R.virtual_rows(vp, vt, P, T, G)
        ko_r, vo_r, so_r, idx_r = R.evict_reference(K, V, score, W, k, tie)
        case = (P, T, k, k * 64 <= P + T - W)
        assert torch.equal(idx.cpu(), idx_r), case
        assert torch.equal(_bits(ko.cpu()), _bits(ko_r)) and torch.equal(_bits(vo.cpu()), _bits(vo_r)), case
        assert torch.equal(_bits(so.cpu()), _bits(so_r)), case
        assert bool((kout[:, :, rows:] == 7).all()) and bool((sout[:, :, rows:] == 7).all())      # nothing behind the k + W rows


# ---- the layer ---------------------------------------------------------------------------------------------------------------
def _layer(dev, B, interval, hq=8, D=64, seed=0, dtype=torch.bfloat16):
    from kvcache_factory_amd import HeavyHitterLayer
    g = torch.Generator().manual_seed(seed)
    layer = HeavyHitterLayer(interval)
    layer.prefill(torch.randn(1, hq, B, D, generator=g).to(dtype).to(dev), torch.randn(1, hq, B, D, generator=g).to(dtype).to(dev), 500)
    layer._sbuf[:, :, :B] = (torch.rand(1, hq, B, generator=g) * 3).to(dev)
    return layer, g


def _checked_step(layer, cluster, q, k, v, scaling):
    """One decode step of the layer checked from the device's own state: the score increment inside the one-step bound, and, when
    the step evicts, the eviction exact against the state it started from.  Returns True if it evicted."""
    P, T = layer.rows()
    t = q.shape[2]
    before = torch.zeros(1, q.shape[1], P + T + t, dtype=torch.float32, device=q.device)
    before[:, :, :P + T] = layer.scores()
    layer.decode_attend(q, k, v, scaling)
    p64, e_ref = R.one_step_bound(q, layer._kbuf, layer._ktail, P, T, scaling)
    R.check_step(before, layer.scores(), p64, e_ref, P + T)
    K, V, score, n0 = layer.keys.clone(), layer.values.clone(), layer.scores(), layer.evictions
    layer.after_decode(cluster, q)
    if layer.evictions == n0:
        return False
    from kvcache_factory_amd import pyramidkv_utils as pu
    B, W = layer._plan
    ko, vo, so, _ = R.evict_reference(K, V, score, W, B - W, pu.TIE_MODE)
    assert layer.rows() == (B, 0)
    assert torch.equal(_bits(layer.keys.cpu()), _bits(ko)) and torch.equal(_bits(layer.values.cpu()), _bits(vo))
    assert torch.equal(_bits(layer.scores().cpu()), _bits(so))
    return True


def test_chain_of_evictions(kvc, gpu_device):
    """Three evictions in a row at the layer level, steps of 1 and 3 tokens, every step and every eviction checked from the
    device's own state (so near-equal scores cannot drift between a reference chain and the device's)."""
    from kvcache_factory_amd import pyramidkv_utils as pu
    cl = pu.H2OKVCluster(window_size=8, max_capacity_prompt=48)
    layer, g = _layer(gpu_device, 48, 16)
    n = 0
    for i in range(44):
        t = 3 if i % 5 == 4 else 1
        q = (torch.randn(1, 8, t, 64, generator=g) * 1.5).to(torch.bfloat16).to(gpu_device)
        k = torch.randn(1, 2, t, 64, generator=g).to(torch.bfloat16).to(gpu_device)
        v = torch.randn(1, 2, t, 64, generator=g).to(torch.bfloat16).to(gpu_device)
        n += _checked_step(layer, cl, q, k, v, 64 ** -0.5)
        assert layer.stored_length() <= 48 + 16 + t - 1
    assert n == layer.evictions >= 3


def test_it_is_h2o(kvc, gpu_device):
    """One early key is aligned with every decode query, another with none (it points the other way): after several evictions
    the first is still in every head's prefix, the second is gone."""
    from kvcache_factory_amd import HeavyHitterLayer, pyramidkv_utils as pu
    B, W, interval, D, hq, hkv = 40, 8, 8, 128, 8, 2
    g = torch.Generator().manual_seed(5)
    u = torch.randn(D, generator=g)
    u = u / u.norm()
    K = torch.randn(1, hq, B, D, generator=g)
    K[:, :, 3], K[:, :, 4] = 6 * u, -6 * u
    K = K.to(torch.bfloat16).to(gpu_device)
    hot, cold = K[:, :, 3].clone(), K[:, :, 4].clone()
    layer = HeavyHitterLayer(interval)
    layer.prefill(K, torch.randn(1, hq, B, D, generator=g).to(torch.bfloat16).to(gpu_device), B)
    cl = pu.H2OKVCluster(window_size=W, max_capacity_prompt=B)
    has = lambda row: (layer.keys == row[:, :, None]).all(-1).any(-1)              # [1, hq]: the row is in the head's cache
    assert bool(has(hot).all()) and bool(has(cold).all())
    for i in range(5 * interval):
        q = (8 * u + torch.randn(1, hq, 1, D, generator=g)).to(torch.bfloat16).to(gpu_device)
        k, v = (torch.randn(1, hkv, 1, D, generator=g).to(torch.bfloat16).to(gpu_device) for _ in range(2))
        layer.decode_attend(q, k, v, D ** -0.5)
        layer.after_decode(cl, q)
    torch.cuda.synchronize()
    assert layer.evictions == 5
    assert bool(has(hot).all()) and not bool(has(cold).any())
    assert bool((layer.scores()[:, :, 0] > 10).all())                              # it went to the front of the top-k order


def test_decode_path_has_no_host_synchronisation(kvc, gpu_device):
    from kvcache_factory_amd import pyramidkv_utils as pu
    cl = pu.H2OKVCluster(window_size=8, max_capacity_prompt=48)
    layer, g = _layer(gpu_device, 48, 16, D=128)
    mk = lambda h: torch.randn(1, h, 1, 128, generator=g).to(torch.bfloat16).to(gpu_device)
    steps = [(mk(8), mk(2), mk(2)) for _ in range(35)]
    for q, k, v in steps[:19]:                                        # one eviction: tail, workspaces and the alternate set exist
        layer.decode_attend(q, k, v, 128 ** -0.5)
        layer.after_decode(cl, q)
    torch.cuda.synchronize()
    assert layer.evictions == 1
    torch.cuda.set_sync_debug_mode("error")
    try:
        for q, k, v in steps[19:]:
            layer.decode_attend(q, k, v, 128 ** -0.5)
            layer.after_decode(cl, q)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert layer.evictions == 2


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["llama", "mistral"])
def test_generate_with_heavy_hitter_cache(kvc, gpu_device, family, monkeypatch):
    """Greedy decoding by hand past three evictions of every layer.  Hooks on the layer's step and eviction: every step's score
    increment against the fp64 restatement from the layer's own rows and the step's post-RoPE queries (one-step bound), every
    eviction exact from the layer's own state; at most B + interval rows per layer; memory flat from the second eviction of every
    layer on; get_seq_length counts every token.  A second run over the same prompt shows no host synchronisation in the
    patched attention forwards of decode steps, evictions included.  (No logits comparison with an uncompressed run: the cache is lossy by design.)"""
    from kvcache_factory_amd import HeavyHitterCache, HeavyHitterLayer, monkeypatch as mp, pyramidkv_utils as pu
    if family == "llama":
        from transformers import LlamaConfig as Cfg, LlamaForCausalLM as Model
        replace = mp.replace_llama
    else:
        from transformers import MistralConfig as Cfg, MistralForCausalLM as Model
        replace = mp.replace_mistral
    extra = dict(sliding_window=None) if family == "mistral" else {}
    cfg = Cfg(hidden_size=4096, intermediate_size=256, num_hidden_layers=3, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
              vocab_size=256, max_position_embeddings=4096, attn_implementation="sdpa", **extra)
    torch.manual_seed(0)
    model = Model(cfg).to(torch.bfloat16).to(gpu_device).eval()
    L, cap, W, interval, new = 300, 64, 8, 32, 140
    ids = torch.randint(0, 256, (1, L), generator=torch.Generator().manual_seed(3)).to(gpu_device)
    steps, evs, peak, mems = {}, {}, {}, []
    orig_attend, orig_evict = HeavyHitterLayer.decode_attend, HeavyHitterLayer._evict
    check = [True]

    def attend(self, q, k, v, scaling):
        if not check[0]:
            return orig_attend(self, q, k, v, scaling)
        P, T = self.rows()
        t = q.shape[2]
        before = torch.zeros(1, q.shape[1], P + T + t, dtype=torch.float32, device=q.device)
        before[:, :, :P + T] = self.scores()
        out = orig_attend(self, q, k, v, scaling)
        p64, e_ref = R.one_step_bound(q, self._kbuf, self._ktail, P, T, scaling)
        R.check_step(before, self.scores(), p64, e_ref, P + T)
        steps[id(self)] = steps.get(id(self), 0) + 1
        peak[id(self)] = max(peak.get(id(self), 0), P + T + t)
        return out

    def evict(self, B, W_, P, T):
        if not check[0]:
            return orig_evict(self, B, W_, P, T)
        K, V, score = self.keys.clone(), self.values.clone(), self.scores()
        orig_evict(self, B, W_, P, T)
        ko, vo, so, _ = R.evict_reference(K, V, score, W_, B - W_, pu.TIE_MODE)
        assert self.rows() == (B, 0) and self.keys.shape[2] == B
        assert torch.equal(_bits(self.keys.cpu()), _bits(ko)) and torch.equal(_bits(self.values.cpu()), _bits(vo))
        assert torch.equal(_bits(self.scores().cpu()), _bits(so))
        evs[id(self)] = evs.get(id(self), 0) + 1

    monkeypatch.setattr(HeavyHitterLayer, "decode_attend", attend)
    monkeypatch.setattr(HeavyHitterLayer, "_evict", evict)
    try:
        replace("h2o")
        for layer in model.model.layers:
            for name, val in (("window_size", W), ("max_capacity_prompt", cap)):
                setattr(layer.self_attn.config, name, val)
        cache = HeavyHitterCache(model.config, interval=interval)
        with torch.no_grad():                  # greedy decoding by hand: generate()'s growing token tensors would hide a flat cache
            logits = model(ids, past_key_values=cache, use_cache=True).logits
            for layer in cache.layers:         # the prefill handed over the H2O compression's own scores
                assert layer.rows() == (cap, 0) and bool((layer.scores()[:, :, :cap - W] > 0).all()) and \
                    float(layer.scores()[:, :, cap - W:].abs().sum()) == 0
            for _ in range(new - 1):
                logits = model(logits[:, -1:].argmax(-1), past_key_values=cache, use_cache=True).logits
                if all(x.evictions >= 2 for x in cache.layers):        # after the second eviction of every layer
                    torch.cuda.synchronize()
                    mems.append(torch.cuda.memory_allocated())
        for layer in cache.layers:
            i = id(layer)
            assert evs.get(i, 0) >= 3 and evs[i] == layer.evictions and steps[i] == new - 1
            assert peak[i] <= cap + interval and layer.stored_length() <= cap + interval
            assert layer.get_seq_length() == L + new - 1 and layer.get_mask_sizes(1)[0] == layer.stored_length() + 1
            assert layer._kbuf.shape[2] == cap and layer._kalt.shape[2] == cap and layer._salt.shape[2] == cap
        assert len(mems) >= interval and len(set(mems)) == 1, sorted(set(mems))
        assert cache.get_seq_length() == L + new - 1
        # the same prompt again on the reset cache, unhooked: no host synchronisation around decode steps, evictions included
        check[0] = False
        cache.reset()
        with torch.no_grad():
            logits = model(ids, past_key_values=cache, use_cache=True).logits
            tok = logits[:, -1:].argmax(-1)
            for _ in range(3):                 # the tail, the step's workspace and transformers' own lazy state exist
                tok = model(tok, past_key_values=cache, use_cache=True).logits[:, -1:].argmax(-1)
            torch.cuda.synchronize()
            # (around the patched attention forwards — projections, RoPE, the scored step, the eviction, o_proj — as the other
            # caches' tests do; what transformers does between them is not this project's)
            hooks = []
            for layer in model.model.layers:
                hooks.append(layer.self_attn.register_forward_pre_hook(lambda *a: torch.cuda.set_sync_debug_mode("error")))
                hooks.append(layer.self_attn.register_forward_hook(lambda *a: torch.cuda.set_sync_debug_mode(0)))
            try:
                for _ in range(2 * interval):
                    tok = model(tok, past_key_values=cache, use_cache=True).logits[:, -1:].argmax(-1)
            finally:
                torch.cuda.set_sync_debug_mode(0)
                for h in hooks:
                    h.remove()
        torch.cuda.synchronize()
        assert all(x.evictions == 2 for x in cache.layers)
    finally:
        replace("fullkv")
