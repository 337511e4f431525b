"""Batched generation over left-padded prompts of unequal length, on the GPU: the per-row decode step (kvc_decode_step_rows)
against fp32 attention, and the cache layer with per-row prefix lengths driven through it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 1e-5}
_INT = {2: torch.int16, 4: torch.int32}


def _bytes_equal(a, b):
    """Byte-for-byte (NaN poison compares equal to itself)."""
    it = _INT[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _fp32_rows_reference(q, kp, vp, rows, kt, vt, T, t, scaling):
    """softmax(q K^T * scaling) V in fp32, batch row b over prefix rows [0, rows[b]) of every head and its KV head's tail rows
    [0, T + i + 1) for the step's token i.  -> [b, hq, t, D]"""
    b, hq, _, D = q.shape
    grp = hq // kt.shape[1]
    ref = torch.empty(b, hq, t, D, dtype=torch.float32, device=q.device)
    for r in range(b):
        P = rows[r]
        K = torch.cat([kp[r, :, :P], kt[r, :, :T + t].repeat_interleave(grp, 0)], 1).float()
        V = torch.cat([vp[r, :, :P], vt[r, :, :T + t].repeat_interleave(grp, 0)], 1).float()
        mask = torch.zeros(t, P + T + t, device=q.device)
        for i in range(t):
            mask[i, P + T + i + 1:] = float("-inf")
        ref[r] = torch.softmax(q[r].float() @ K.transpose(1, 2) * scaling + mask, -1) @ V
    return ref


@pytest.mark.parametrize("dtype,D,hq,hkv,rows,T,t", [
    (torch.bfloat16, 128, 32, 8, [2056, 40, 0, 1032], 300, 1),
    (torch.bfloat16, 128, 32, 8, [1, 63, 64, 65], 0, 3),
    (torch.bfloat16, 64, 8, 2, [63, 520, 1, 65, 0, 64], 37, 3),
    (torch.float16, 64, 8, 2, [2056, 40, 0, 1032], 37, 3),
    (torch.float16, 128, 4, 4, [0, 1, 63, 64, 65, 300, 5], 300, 1),
    (torch.float32, 128, 8, 2, [65, 64, 1, 0], 37, 1),
    (torch.float32, 64, 4, 4, [2056, 40, 0, 1032], 0, 1),
    (torch.float32, 64, 32, 8, [1032, 0, 65], 300, 3),
    (torch.bfloat16, 128, 8, 2, [0, 0], 0, 1),
])
def test_decode_step_rows_vs_fp32_attention(kvc, gpu_device, dtype, D, hq, hkv, rows, T, t):
    """kvc_decode_step_rows: batch row b attends to prefix rows [0, rows[b]) and the shared-length tail.  Against an fp32
    reference from the same inputs, tolerance of test_decode_step_vs_reference_shaped_attention (2^-7 bf16, 2^-10 fp16, 1e-5
    fp32, times max(1, max |ref|)).  Every prefix row at or past rows[b] (and every spare row) is NaN before the call: a NaN in
    the output is a row the kernel must not have read.  The tail holds the appended rows byte for byte and nothing else in it
    changes.  The call is repeated over a workspace filled with NaN and must give the same bytes (a split that had no rows for
    a short batch row must not be merged from stale workspace)."""
    b, bound = len(rows), max(rows)
    g = torch.Generator().manual_seed(sum(rows) + T + t)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(dtype).to(gpu_device)      # noqa: E731
    q, kn, vn = rn(b, hq, t, D), rn(b, hkv, t, D), rn(b, hkv, t, D)
    kp, vp = rn(b, hq, bound + 7, D), rn(b, hq, bound + 7, D)
    for r in range(b):
        kp[r, :, rows[r]:] = float("nan")
        vp[r, :, rows[r]:] = float("nan")
    kt, vt = rn(b, hkv, T + t + 4, D), rn(b, hkv, T + t + 4, D)
    kt[:, :, T + t:] = float("nan")
    vt[:, :, T + t:] = float("nan")
    kt0, vt0 = kt.clone(), vt.clone()
    rows_b = torch.tensor(rows, dtype=torch.int32, device=gpu_device)
    out = kvc.decode_step_rows(q, kn, vn, kp, vp, rows_b, bound, kt, vt, T, D ** -0.5)
    assert out.shape == (b, t, hq, D)
    assert not torch.isnan(out.float()).any(), "the kernel read a prefix row it must not see"
    for tail, tail0, new in ((kt, kt0, kn), (vt, vt0, vn)):
        assert _bytes_equal(tail[:, :, T:T + t], new)
        assert _bytes_equal(tail[:, :, :T], tail0[:, :, :T]) and _bytes_equal(tail[:, :, T + t:], tail0[:, :, T + t:])
    ref = _fp32_rows_reference(q, kp, vp, rows, kt, vt, T, t, D ** -0.5)
    err = float((out.transpose(1, 2).float() - ref).abs().max())
    bound_err = TOL[dtype] * max(1.0, float(ref.abs().max()))
    print(f"max |out - ref| = {err:.3e} (allowed {bound_err:.3e})")
    assert err <= bound_err
    # the same call over a poisoned workspace
    ws = kvc.workspace(gpu_device, 1)
    ws.fill_(0xFF)                                                          # every fp32 word a NaN
    out2 = kvc.decode_step_rows(q, kn, vn, kp, vp, rows_b, bound, kt, vt, T, D ** -0.5)
    assert _bytes_equal(out2, out)
    # entries beyond the bound are clamped to it, negative ones to 0
    wild = rows_b.clone()
    wild[rows.index(bound)] = 2 ** 30
    wild[rows.index(min(rows))] = -5 if min(rows) == 0 else min(rows)
    out3 = kvc.decode_step_rows(q, kn, vn, kp, vp, wild, bound, kt, vt, T, D ** -0.5)
    assert _bytes_equal(out3, out)


def test_decode_step_rows_equals_decode_step_for_uniform_rows(kvc, gpu_device):
    """With every entry equal to the bound the batch step sees what kvc_decode_step2 sees: same tolerance against each other."""
    g = torch.Generator().manual_seed(5)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(torch.bfloat16).to(gpu_device)      # noqa: E731
    b, hq, hkv, D, P, T = 3, 32, 8, 128, 520, 37
    q, kn, vn, kp, vp = rn(b, hq, 1, D), rn(b, hkv, 1, D), rn(b, hkv, 1, D), rn(b, hq, P, D), rn(b, hq, P, D)
    kt, vt = rn(b, hkv, T + 8, D), rn(b, hkv, T + 8, D)
    kt2, vt2 = kt.clone(), vt.clone()
    a = kvc.decode_step_rows(q, kn, vn, kp, vp, torch.full((b,), P, dtype=torch.int32, device=gpu_device), P, kt, vt, T, D ** -0.5)
    c = kvc.decode_step(q, kn, vn, kp, vp, P, kt2, vt2, T, D ** -0.5)
    assert torch.equal(kt, kt2) and torch.equal(vt, vt2)
    assert float((a.float() - c.float()).abs().max()) <= 2.0 ** -7 * max(1.0, float(c.float().abs().max()))


# ---- per-row compression on the device ------------------------------------------------------------------------------------------
HQ, HKV, D, CAP, W = 8, 2, 128, 128, 8
LENS = (100, 200, 700)                # below the cap; PyramidKV's middle branch (cap <= L < 2 (cap - W)); above 2 (cap - W)


def _cluster(name, layer_idx=0, n_layers=4):
    from kvcache_factory_amd import pyramidkv_utils as pu
    kw = dict(window_size=W, max_capacity_prompt=CAP, kernel_size=7, pooling="maxpool")
    if name == "snapkv":
        return pu.SnapKVCluster(**kw)
    if name == "pyramidkv":
        return pu.PyramidKVCluster(num_hidden_layers=n_layers, layer_idx=layer_idx, **kw)
    if name == "streamingllm":
        return pu.StreamingLLMKVCluster(**kw)
    if name == "h2o":
        return pu.H2OKVCluster(**kw)
    return pu.L2NormCluster(max_capacity_prompt=CAP, layer_idx=layer_idx, skip_layers=[])


@pytest.mark.parametrize("tie_mode", ["torch_cpu", "canonical"])
@pytest.mark.parametrize("method,layer_idx", [("snapkv", 0), ("pyramidkv", 0), ("pyramidkv", 3), ("streamingllm", 0), ("h2o", 0), ("l2norm", 0)])
def test_each_row_keeps_what_the_prompt_keeps_alone_on_the_device(kvc, gpu_device, monkeypatch, method, layer_idx, tie_mode):
    """pyramidkv_utils.prefill_rows with the real kernels: row b of the layer's buffers is, byte for byte, what a bsz = 1 update_kv
    returns for that prompt alone (pass-through rows repeat_kv-expanded); pad columns hold garbage.  Both tie modes, through the
    grouped PrefillBatch flush on the side stream and through direct per-row calls."""
    from kvcache_factory_amd import pyramidkv_utils as pu
    from kvcache_factory_amd.cache import CompressedDynamicLayer
    monkeypatch.setattr(pu, "TIE_MODE", tie_mode)
    g = torch.Generator().manual_seed(41 + layer_idx)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(torch.bfloat16)      # noqa: E731
    L = max(LENS)
    rows = [(rn(1, HQ, n, D), rn(1, HKV, n, D), rn(1, HKV, n, D)) for n in LENS]
    Q, K, V = rn(3, HQ, L, D) * 30, rn(3, HKV, L, D) * 30, rn(3, HKV, L, D) * 30
    for b, (q, k, v) in enumerate(rows):
        Q[b, :, L - LENS[b]:], K[b, :, L - LENS[b]:], V[b, :, L - LENS[b]:] = q[0], k[0], v[0]
    Q, K, V = Q.to(gpu_device), K.to(gpu_device), V.to(gpu_device)
    starts = tuple(L - n for n in LENS)
    cluster = _cluster(method, layer_idx)
    for parked in (True, False):
        layer, pending = CompressedDynamicLayer(), (pu.PrefillBatch() if parked else None)
        pu.prefill_rows(cluster, layer, K, Q, V, starts, HQ // HKV, pending)
        if parked:
            pending.flush(overlap=True)
            pending.settle()
        lengths = layer.row_lengths().tolist()
        for b, (q, k, v) in enumerate(rows):
            q, k, v = q.to(gpu_device), k.to(gpu_device), v.to(gpu_device)
            kc, vc = cluster.update_kv(k, q, v, None, HQ // HKV)
            if kc is k:
                kc, vc = k.repeat_interleave(HQ // HKV, 1), v.repeat_interleave(HQ // HKV, 1)
            assert lengths[b] == kc.shape[2]
            assert _bytes_equal(layer._kbuf[b:b + 1, :, :lengths[b]], kc), (parked, b)
            assert _bytes_equal(layer._vbuf[b:b + 1, :, :lengths[b]], vc), (parked, b)
        assert lengths[0] == LENS[0] and layer.has_holes()


# ---- model level -----------------------------------------------------------------------------------------------------------------
def _llama(gpu_device):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=256, num_hidden_layers=3, num_attention_heads=32, num_key_value_heads=8,
                      head_dim=128, vocab_size=256, max_position_embeddings=4096, attn_implementation="sdpa", eos_token_id=None,
                      pad_token_id=0, bos_token_id=None)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).to(gpu_device).eval()


def _set_knobs(model, cap, window=8):
    for layer in model.model.layers:
        for name, val in (("window_size", window), ("max_capacity_prompt", cap), ("kernel_size", 7), ("pooling", "maxpool")):
            setattr(layer.self_attn.config, name, val)


def _padded(lens, gpu_device, seed=5):
    g = torch.Generator().manual_seed(seed)
    L = max(lens)
    ids = torch.zeros(len(lens), L, dtype=torch.long)
    mask = torch.zeros(len(lens), L, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, L - n:] = torch.randint(1, 256, (n,), generator=g)
        mask[b, L - n:] = 1
    return ids.to(gpu_device), mask.to(gpu_device)


def _teacher_forced(model, ids, mask, tokens, cache=None):
    """Direct forwards as generate() makes them (explicit mask and per-row positions); row b is fed tokens[b][j] at step j.
    -> logits [step][b, vocab] (step 0: the prefill's), the cache."""
    from transformers import DynamicCache
    cache = DynamicCache() if cache is None else cache
    lens = mask.sum(-1)
    with torch.no_grad():
        out = [model(ids, attention_mask=mask, position_ids=(mask.cumsum(-1) - 1).clamp(min=0), past_key_values=cache,
                     use_cache=True).logits[:, -1].float()]
        for j in range(tokens.shape[1]):
            mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
            out.append(model(tokens[:, j:j + 1], attention_mask=mask, position_ids=(lens + j)[:, None], past_key_values=cache,
                             use_cache=True).logits[:, -1].float())
    return out, cache


def _assert_close(a, b, what):
    """Every step, every row: |a - b| <= 3e-2 * max |b| (the bound of test_decode_logits_vs_oracle_built_cache)."""
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        for r in range(x.shape[0]):
            err, scale = float((x[r] - y[r]).abs().max()), float(y[r].abs().max())
            print(f"{what} step {j} row {r}: max |logit diff| {err:.4f}, allowed {3e-2 * scale:.4f}")
            assert err <= 3e-2 * scale, (what, j, r, err, scale)


PROMPTS = (500, 100, 60)              # above 2 (cap - W); PyramidKV's middle branch; below the cap (passed through)


@pytest.mark.parametrize("method", ["snapkv", "pyramidkv", "streamingllm"])
def test_generate_over_a_left_padded_batch(kvc, gpu_device, monkeypatch, method):
    """generate() with attention_mask over three left-padded prompts (500, 100 and 60 tokens; max_capacity_prompt 72, window 8) on
    the Llama of test_decode_logits_vs_oracle_built_cache:
      (a) the fused batched step was taken (every layer in the SPLIT form, kvc_decode_step_rows called once per layer and step);
      (b) for every row, the layer's rows equal the CPU oracle's output for that row's slice of the Q / K / V that reached the
          per-row prefill in the same run, byte for byte (the short prompt: passed through, repeat_kv-expanded);
      (c) with the tokens generate() chose fed to direct forwards (teacher forcing: every step of every row is compared), the
          logits of the fused form are within 3e-2 * max|logit| of the same run with BATCH_DECODE off (the reference-shaped form
          with the layer's own mask), and generate()'s own scores are within the same bound of the fused direct run."""
    import cpu_compress
    from kvcache_factory_amd import monkeypatch as mp, pyramidkv_utils as pu
    model = _llama(gpu_device)
    ids, mask = _padded(PROMPTS, gpu_device)
    cap, steps = 72, 5
    seen, calls = [], []
    real_prefill, real_step = pu.prefill_rows, kvc.decode_step_rows

    def spy_prefill(cluster, layer, K, Q, V, starts, groups, pending=None):
        seen.append((cluster, layer, K.cpu(), Q.cpu(), V.cpu(), starts))
        return real_prefill(cluster, layer, K, Q, V, starts, groups, pending)

    def spy_step(*a, **kw):
        calls.append(1)
        return real_step(*a, **kw)
    try:
        mp.replace_llama(method)
        _set_knobs(model, cap)
        monkeypatch.setattr(pu, "prefill_rows", spy_prefill)
        monkeypatch.setattr(kvc, "decode_step_rows", spy_step)
        with torch.no_grad():
            gen = model.generate(ids, attention_mask=mask, max_new_tokens=steps, do_sample=False, use_cache=True,
                                 return_dict_in_generate=True, output_scores=True)
        monkeypatch.setattr(pu, "prefill_rows", real_prefill)
        # (a)
        layers = gen.past_key_values.layers
        assert len(seen) == 3 and len(calls) == 3 * (steps - 1)              # (the last token is not fed back)
        assert all(la._split and type(la).__name__ == "CompressedDynamicLayer" for la in layers)
        # (b)
        for cluster, layer, K, Q, V, starts in seen:
            assert starts == tuple(max(PROMPTS) - n for n in PROMPTS)
            lengths = layer.row_lengths().tolist()
            assert layer.get_seq_length() == max(PROMPTS) + steps - 1 and lengths[2] == PROMPTS[2] and layer.has_holes()
            for b, s in enumerate(starts):
                k, q, v = K[b:b + 1, :, s:].contiguous(), Q[b:b + 1, :, s:].contiguous(), V[b:b + 1, :, s:].contiguous()
                if PROMPTS[b] < cap:
                    kc, vc = k.repeat_interleave(4, 1), v.repeat_interleave(4, 1)
                else:
                    kc, vc = cpu_compress.oracle_compress(cluster._method, q if method != "streamingllm" else None, k, v, 8,
                                                          cluster._budget(PROMPTS[b]), 7, "maxpool", pu.TIE_MODE, n_q_heads=32)
                assert lengths[b] == kc.shape[2]
                assert _bytes_equal(layer._kbuf[b:b + 1, :, :lengths[b]].cpu(), kc), (method, b)
                assert _bytes_equal(layer._vbuf[b:b + 1, :, :lengths[b]].cpu(), vc), (method, b)
        # (c)
        tokens = gen.sequences[:, ids.shape[1]:]
        fused, cache_f = _teacher_forced(model, ids, mask, tokens)
        assert all(la._split for la in cache_f.layers)
        monkeypatch.setattr(pu, "BATCH_DECODE", False)
        shaped, cache_s = _teacher_forced(model, ids, mask, tokens)
        assert not any(la._split for la in cache_s.layers) and all(la.has_holes() for la in cache_s.layers)
    finally:
        mp.replace_llama("fullkv")
    _assert_close(fused, shaped, f"{method} fused vs reference-shaped")
    _assert_close([s.float() for s in gen.scores], fused[:steps], f"{method} generate() vs direct fused")


@pytest.mark.parametrize("form", ["fused", "reference_shaped"])
def test_all_rows_passed_through_agree_with_stock_transformers(kvc, gpu_device, monkeypatch, form):
    """A cap above every length: nothing is evicted, so the patched model on the padded batch must agree with the UNPATCHED model on
    the same batch, step by step (3e-2 * max|logit|), in the fused form and with BATCH_DECODE off — the new step and the layer's
    own mask against transformers' masking.  (The reference-shaped case also held before batches were supported: nothing was
    evicted, so transformers' own mask still fitted.)"""
    from kvcache_factory_amd import monkeypatch as mp, pyramidkv_utils as pu
    model = _llama(gpu_device)
    ids, mask = _padded((300, 120, 37), gpu_device, seed=9)
    with torch.no_grad():
        tokens = model.generate(ids, attention_mask=mask, max_new_tokens=5, do_sample=False, use_cache=True)[:, ids.shape[1]:]
    stock, _ = _teacher_forced(model, ids, mask, tokens)
    try:
        mp.replace_llama("snapkv")
        _set_knobs(model, 1024)
        if form == "reference_shaped":
            monkeypatch.setattr(pu, "BATCH_DECODE", False, raising=False)
        got, cache = _teacher_forced(model, ids, mask, tokens)
    finally:
        mp.replace_llama("fullkv")
    if form == "fused":
        assert all(la._split and la.row_lengths().tolist() == [300, 120, 37] for la in cache.layers)
    else:
        assert not any(la._split for la in cache.layers)
    _assert_close(got, stock, f"{form} vs stock")


def test_batched_decode_steps_do_not_synchronise_and_a_padded_prefill_reads_once(kvc, gpu_device):
    """Decode steps of the plain cache for a batch with unequal rows under sync debug mode "error"; and the prefill of ALL layers
    of a padded batch under mode "warn": the attention modules are called directly (the mask transformers builds, and whatever
    the model does around the attention modules, is outside what this package adds), and the warnings are counted — exactly one,
    the read of the mask's geometry at layer 0."""
    import warnings
    from transformers import DynamicCache
    from transformers.masking_utils import create_causal_mask
    from kvcache_factory_amd import monkeypatch as mp
    model = _llama(gpu_device)
    ids, mask = _padded(PROMPTS, gpu_device)
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    hidden = model.model.embed_tokens(ids)
    cos_sin = model.model.rotary_emb(hidden, pos)
    cache = DynamicCache()
    m4 = create_causal_mask(config=model.config, inputs_embeds=hidden, attention_mask=mask, past_key_values=cache, position_ids=pos)
    assert torch.is_tensor(m4) and m4.dim() == 4
    try:
        mp.replace_llama("pyramidkv")
        _set_knobs(model, 72)
        with torch.no_grad():
            model.model.layers[0].self_attn(hidden, position_embeddings=cos_sin, attention_mask=m4, past_key_values=DynamicCache())  # warm-up
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("warn")
            try:
                with warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    for layer in model.model.layers:
                        layer.self_attn(hidden, position_embeddings=cos_sin, attention_mask=m4, past_key_values=cache)
            finally:
                torch.cuda.set_sync_debug_mode(0)
            syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
            print("synchronising calls during the padded prefill:", syncs)
            assert len(syncs) == 1, syncs
            assert all(la.has_holes() for la in cache.layers)
            step = torch.randn(3, 1, 4096, device=gpu_device).to(torch.bfloat16)
            cs = model.model.rotary_emb(step, mask.sum(-1)[:, None])
            for layer in model.model.layers:                                  # warm-up: tails and workspace exist
                layer.self_attn(step, position_embeddings=cs, attention_mask=None, past_key_values=cache)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                for _ in range(4):
                    for layer in model.model.layers:
                        layer.self_attn(step, position_embeddings=cs, attention_mask=None, past_key_values=cache)
            finally:
                torch.cuda.set_sync_debug_mode(0)
            torch.cuda.synchronize()
    finally:
        mp.replace_llama("fullkv")
    assert all(la._split and la._tail == 5 for la in cache.layers)


def test_beam_search_over_a_padded_batch(kvc, gpu_device):
    """num_beams = 2 over two left-padded prompts: runs, and every layer's row lengths still belong to its buffers — each beam's
    entry is the length of the prompt it descends from, and rows at or past it were never written by a prefill of that length."""
    from kvcache_factory_amd import monkeypatch as mp
    model = _llama(gpu_device)
    ids, mask = _padded((200, 50), gpu_device, seed=11)
    try:
        mp.replace_llama("snapkv")
        _set_knobs(model, 72)
        with torch.no_grad():
            gen = model.generate(ids, attention_mask=mask, max_new_tokens=4, do_sample=False, num_beams=2, use_cache=True,
                                 return_dict_in_generate=True)
    finally:
        mp.replace_llama("fullkv")
    assert gen.sequences.shape == (2, 204)
    for la in gen.past_key_values.layers:
        assert la._kbuf.shape[0] == 4 and la.row_lengths().tolist() == [72, 72, 50, 50] and la._stored == 72 and la.has_holes()
        assert la.get_seq_length() == 203
